"""fp64 numpy restatement of STOI as `stoi(xref, xest, fs)` computes it (score_audio.m:231) -- the contract
csrc/stoi.hip implements.  No scipy, no GPU.

[STOI-memory]: the STOI toolbox (Taal, Hendriks, Heusdens, Jensen, "An algorithm for intelligibility prediction
of time-frequency weighted noisy speech", IEEE TASLP 19(7), 2011) is not part of the reference repository (its
download_toolboxes.sh fetches it); this is a restatement of the published algorithm.  x = reference (clean),
y = estimate.  Constants: fs 10000, frame 256, FFT 512, 15 bands from 150 Hz, segments of 30 frames,
beta = -15 dB, 40 dB silence range.  Indices are 0-based.

1. Resample to 10 kHz as Matlab resample(x, 10000, fs) with N = 10, Kaiser beta = 5: p/q = 10000/fs reduced,
   L = 2 * 10 * max(p, q) + 1 taps h = kaiser(L, 5) * sinc((i - (L-1)/2) / max(p,q)) / max(p,q), h <- p h / sum h,
   y[m] = sum_k x[k] h[q m + (L-1)/2 - p k] for m < ceil(len p / q).
2. Silent frames: frames at 128 j for every start <= len - 257, window Matlab hanning(256); energy
   e_j = 20 log10(||x_j w|| / 16); keep iff e_j - max(e) + 40 > 0; the kept windowed frames of x and of y are
   overlap-added at 128 c (c = 0, 1, ...).
3. Band envelopes: the same framing and window on the compacted signals, 512-point FFT, X_j = sqrt of the sum of
   |X_k|^2 over band j's bins [lo_j, hi_j).
4. For every segment of 30 frames ending at m = 29 .. n_frames - 1 and band j: alpha = sqrt(sum X^2 / sum Y^2),
   Y' = min(alpha Y, X (1 + 10^(-beta/20))), d = corr(X, Y') (centred, divided by the norms, no epsilon).
   STOI = mean d.
5. Matlab's edge semantics, not pystoi's: fewer than 30 frames -> NaN (mean of an empty set); min ignores NaN;
   a zero-variance vector -> NaN, which propagates.
"""
import math

import numpy as np

FS = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
J = 15
MN = 150.0
N_SEG = 30
BETA = -15.0
DYN_RANGE = 40.0
CLIP = 1.0 + 10.0 ** (-BETA / 20.0)


def rate(fs):
    """(p, q) = 10000 / fs reduced."""
    g = math.gcd(FS, int(fs))
    return FS // g, int(fs) // g


def _i0(x):
    """Modified Bessel function of the first kind, order 0 (power series)."""
    x = np.asarray(x, dtype=np.float64)
    q = 0.25 * x * x
    term = np.ones_like(x)
    s = np.ones_like(x)
    for k in range(1, 80):
        term = term * q / (k * k)
        s = s + term
    return s


def kaiser(L, beta):
    n = np.arange(L, dtype=np.float64)
    r = (n - (L - 1) / 2.0) / ((L - 1) / 2.0)
    return _i0(beta * np.sqrt(np.maximum(0.0, 1.0 - r * r))) / _i0(beta)


def resample_filter(fs):
    """Matlab resample's default filter for 10000/fs: (h, p, q, Lhalf)."""
    p, q = rate(fs)
    mpq = max(p, q)
    L = 2 * 10 * mpq + 1
    half = (L - 1) // 2
    h = kaiser(L, 5.0) * np.sinc((np.arange(L) - half) / mpq) / mpq
    h = p * h / h.sum()
    return h, p, q, half


def resample(x, fs):
    """x (1-D) at fs -> 10 kHz, Matlab resample(x, 10000, fs) written out."""
    x = np.asarray(x, dtype=np.float64)
    if int(fs) == FS:
        return x.copy()
    h, p, q, half = resample_filter(fs)
    L = len(h)
    lx = len(x)
    ny = -(-lx * p // q)
    m = np.arange(ny, dtype=np.int64)[:, None]
    k = (q * m + half) // p - np.arange(L // p + 2, dtype=np.int64)[None, :]   # every k with h index >= 0
    t = q * m + half - p * k
    ok = (t >= 0) & (t < L) & (k >= 0) & (k < lx)
    return np.where(ok, x[np.clip(k, 0, max(lx - 1, 0))] * h[np.clip(t, 0, L - 1)], 0.0).sum(axis=1)


def hanning(n):
    """Matlab hanning(n): the symmetric Hann window without its zero end points."""
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(1, n + 1) / (n + 1)))


def frame_starts(length):
    """Matlab 1:K:(length - N) in 0-based starts: every start <= length - 257."""
    return np.arange(0, max(length - N_FRAME, 0), HOP)


def frame_energies(x):
    """e_j = 20 log10(||x_j w|| / sqrt(N)) of the silence detector (dB)."""
    w = hanning(N_FRAME)
    st = frame_starts(len(x))
    with np.errstate(divide="ignore"):
        return np.array([20.0 * np.log10(np.linalg.norm(x[s:s + N_FRAME] * w) / np.sqrt(N_FRAME)) for s in st])


def remove_silent_frames(x, y):
    """(x_sil, y_sil, keep): overlap-add of the frames of x within DYN_RANGE dB of its loudest (x decides for
    both)."""
    w = hanning(N_FRAME)
    st = frame_starts(len(x))
    e = frame_energies(x)
    if len(e) == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, dtype=bool)
    with np.errstate(invalid="ignore"):
        keep = (e - e.max() + DYN_RANGE) > 0
    n = int(keep.sum())
    if n == 0:
        return np.zeros(0), np.zeros(0), keep
    out_len = HOP * (n - 1) + N_FRAME
    xs, ys = np.zeros(out_len), np.zeros(out_len)
    c = 0
    for j, s in enumerate(st):
        if keep[j]:
            xs[HOP * c:HOP * c + N_FRAME] += x[s:s + N_FRAME] * w
            ys[HOP * c:HOP * c + N_FRAME] += y[s:s + N_FRAME] * w
            c += 1
    return xs, ys, keep


def third_octave_bands(fs=FS, nfft=NFFT, num_bands=J, mn=MN):
    """(lo, hi) bin index pairs: the FFT bins nearest (first on ties) to each band's edges."""
    f = np.linspace(0, fs, nfft + 1)[:nfft // 2 + 1]
    k = np.arange(num_bands, dtype=np.float64)
    cf = 2.0 ** (k / 3.0) * mn
    fl = np.sqrt(2.0 ** (k / 3.0) * mn * 2.0 ** ((k - 1) / 3.0) * mn)
    fr = np.sqrt(2.0 ** (k / 3.0) * mn * 2.0 ** ((k + 1) / 3.0) * mn)
    lo = [int(np.argmin((f - v) ** 2)) for v in fl]
    hi = [int(np.argmin((f - v) ** 2)) for v in fr]
    return list(zip(lo, hi)), cf


BANDS = third_octave_bands()[0]


def band_envelopes(x):
    """[n_frames, 15] band amplitudes of the windowed 512-point STFT of a compacted signal."""
    w = hanning(N_FRAME)
    st = frame_starts(len(x))
    out = np.zeros((len(st), J))
    for i, s in enumerate(st):
        X = np.fft.fft(x[s:s + N_FRAME] * w, NFFT)
        p = np.abs(X) ** 2
        for j, (lo, hi) in enumerate(BANDS):
            out[i, j] = np.sqrt(p[lo:hi].sum())
    return out


def segment_scores(X, Y):
    """d [n_frames - 29, 15] for the envelopes X, Y [n_frames, 15] (Matlab min: NaN ignored)."""
    nf = X.shape[0]
    d = np.zeros((max(nf - N_SEG + 1, 0), J))
    with np.errstate(divide="ignore", invalid="ignore"):
        for m in range(N_SEG - 1, nf):
            xs = X[m - N_SEG + 1:m + 1]
            ys = Y[m - N_SEG + 1:m + 1]
            alpha = np.sqrt((xs ** 2).sum(0) / (ys ** 2).sum(0))
            yp = np.fmin(ys * alpha, xs * CLIP)
            xn = xs - xs.mean(0)
            yn = yp - yp.mean(0)
            xn = xn / np.sqrt((xn ** 2).sum(0))
            yn = yn / np.sqrt((yn ** 2).sum(0))
            d[m - N_SEG + 1] = (xn * yn).sum(0)
    return d


def stoi(x, y, fs, return_parts=False):
    """STOI of estimate y against reference x (1-D arrays at fs), fp64."""
    x = resample(np.asarray(x, dtype=np.float64), fs)
    y = resample(np.asarray(y, dtype=np.float64), fs)
    e = frame_energies(x)
    xs, ys, keep = remove_silent_frames(x, y)
    X, Y = band_envelopes(xs), band_envelopes(ys)
    d = segment_scores(X, Y)
    with np.errstate(invalid="ignore"):
        val = float(d.mean()) if d.size else float("nan")
    if return_parts:
        return val, dict(keep=keep, energies=e, env_ref=X, env_est=Y, d=d, x10k=x, y10k=y)
    return val


def speech_like(rng, n, fs, gaps=True):
    """A deterministic speech-like test signal: a harmonic tone (f0 gliding between about 100 and 220 Hz, harmonics
    falling off as 1/h up to 4 kHz) amplitude-modulated at a syllable rate (~4 Hz), with low-level stretches the
    silence detector removes, over a -70 dB noise floor."""
    t = np.arange(n) / fs
    f0 = 160.0 + 60.0 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 2 * np.pi))
    ph = 2 * np.pi * np.cumsum(f0) / fs
    s = np.zeros(n)
    for hh in range(1, int(4000 // 100) + 1):
        s += np.where(hh * f0 < 0.45 * fs, 1.0 / hh, 0.0) * np.sin(hh * ph + rng.uniform(0, 2 * np.pi))
    syl = 0.5 * (1.0 - np.cos(2 * np.pi * 4.0 * t + rng.uniform(0, 2 * np.pi)))
    env = 0.05 + 0.95 * syl
    if gaps:
        # word gaps: ~250 ms at 1e-3 of the level every ~1.1 s
        g = np.ones(n)
        period = int(1.1 * fs)
        start = int(rng.integers(0, period))
        while start < n:
            g[start:start + int(0.25 * fs)] = 1e-3
            start += period
        env = env * g
    s = 0.1 * s * env
    return s + 1e-4 * 0.1 * rng.standard_normal(n)


def add_noise(rng, x, snr_db):
    noise = rng.standard_normal(len(x))
    noise *= np.sqrt(np.sum(x ** 2) / np.sum(noise ** 2) / 10.0 ** (snr_db / 10.0))
    return x + noise


def lowpass_delay(x, delay):
    """A low-passed (3-tap [1 2 1] / 4) copy delayed by `delay` samples."""
    y = np.convolve(x, np.array([0.25, 0.5, 0.25]))[:len(x)]
    return np.concatenate([np.zeros(delay), y[:len(x) - delay]])
