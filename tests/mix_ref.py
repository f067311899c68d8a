"""The definition of include/drnmf_mix.h in numpy fp64: what the device-side mixer is checked against.

    g, noisy = mix_one(speech, noise_or_None, offset, snr_db)

speech / noise: 1-D int16 (a sample is v / 32768, exact in float32) or float32 arrays.  g is fp64 (the kernel
rounds it once to float32), noisy = s + g * seg in fp64."""
import numpy as np


def as_float(v):
    """The float32 sample values as fp64."""
    v = np.asarray(v)
    if v.dtype == np.int16:
        return v.astype(np.float64) / 32768.0
    assert v.dtype == np.float32, v.dtype
    return v.astype(np.float64)


def segment(noise, offset, n):
    """seg[k] = noise[(offset mod L + k) mod L], k < n."""
    z = as_float(noise)
    L = z.shape[0]
    o = int(offset) % L                         # Python's %: in [0, L) for a negative offset as well
    return z[(o + np.arange(n, dtype=np.int64)) % L]


def gain(es, en, snr_db):
    if es == 0.0 or en == 0.0 or not np.isfinite(snr_db):
        return 0.0
    with np.errstate(over='ignore', invalid='ignore'):
        g = np.sqrt(np.float64(es) / np.float64(en)) * np.float64(10.0) ** (-np.float64(snr_db) / 20.0)
        if not np.isfinite(g) or not np.isfinite(np.float32(g)):
            return 0.0
    return float(g)


def mix_one(speech, noise, offset, snr_db):
    """(g, noisy, seg) of one signal; noise None or empty: no noise (g = 0)."""
    s = as_float(speech)
    if noise is None or len(noise) == 0:
        return 0.0, s.copy(), np.zeros_like(s)
    seg = segment(noise, offset, s.shape[0])
    g = gain(float(np.sum(s * s)), float(np.sum(seg * seg)), float(snr_db))
    return g, s + g * seg, seg


def realised_snr_db(speech_f64, noisy_f64):
    d = noisy_f64 - speech_f64
    return 10.0 * np.log10(np.sum(speech_f64 * speech_f64) / np.sum(d * d))
