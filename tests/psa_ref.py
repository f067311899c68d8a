"""The fp64 reference of the training targets of include/drnmf_target.h, and the waveform pairs both of their test
files share (test_target_host.py on the CPU, test_gpu_target.py on the MI355X).  numpy and the oracle only: no GPU
needed.

The clean members are rows of stft_hops_ref.signals, so their fp64 spectra are stft_hops_ref.spectra and the
bound on a device spectrum is that module's TOL_FWD; neither is restated here.
"""
import functools

import numpy as np

import stft_hops_ref as R
from oracle import drnmf_oracle as O

TARGETS = ("psa", "tpsa")
MAXLEN = 23           # below the longest frame count of every size (37 at (2048, 512)): sequences are cut


def magnitude(X, m_x=None):
    """m_x as float64: the one given, or |X| correctly rounded."""
    if m_x is not None:
        return np.asarray(m_x, dtype=np.float64)
    X = np.asarray(X, dtype=np.complex128)
    return np.sqrt(X.real.astype(np.longdouble) ** 2 + X.imag.astype(np.longdouble) ** 2).astype(np.float64)


def project(S, X, m_x=None):
    """p = Re(S conj X) / m_x = (re_s re_x + im_s im_x) / m_x where m_x > 0, 0 where m_x == 0, as float64.  S, X:
    complex spectra of the clean and of the noisy member (conjugating both changes nothing); m_x: the noisy
    magnitude to divide by (default |X|).  The numerator is formed in long double, so that the float64 result is
    the rounded quotient and not three float64 roundings away from it."""
    S, X = np.asarray(S, dtype=np.complex128), np.asarray(X, dtype=np.complex128)
    ld = lambda a: a.astype(np.longdouble)
    m = ld(magnitude(X, m_x))
    num = ld(S.real) * ld(X.real) + ld(S.imag) * ld(X.imag)
    return np.divide(num, m, out=np.zeros_like(num), where=m > 0).astype(np.float64)


def target(kind, S, X, m_x=None):
    """'psa': p.  'tpsa': min(max(p, 0), m_x)."""
    p = project(S, X, m_x)
    if kind == "psa":
        return p
    assert kind == "tpsa", kind
    return np.minimum(np.maximum(p, 0.0), magnitude(X, m_x))


# the kind of pair each clean length of stft_hops_ref.lengths gets (the one-sample signal is left out: 6 pairs)
def _kinds(hop):
    return {hop - 1: "negated",        # shorter than a window; clean = -noisy
            hop: "longer",             # an exact multiple of the hop; the noisy member is 2 hop + 44 samples longer
            hop + 1: "same",           # clean = noisy
            3 * hop + 7: "noise",      # noisy = clean + noise of equal length
            9999: "early",             # ... which ends inside the last frames (as early as the frame count allows)
            16001: "zeros"}            # ... with a stretch of N + hop + 5 exact zeros: whole frames with m_x == 0


def _noise(rng, n, int16):
    if int16:
        return rng.integers(-3000, 3000, size=n).astype(np.int16)         # |clean + noise| < 2^15
    return (0.1 * rng.standard_normal(n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pairs(N, hop, int16):
    """(kinds, noisy, clean, X64, S64) of a size and input type: lists over the six pairs; X64, S64 complex128
    [F, nf] with nf the CLEAN member's frame count (the noisy spectrum cut to it).  Never modified."""
    lens, pcm = R.signals(N, hop, int16)
    spectra = R.spectra(N, hop, int16)
    rng = np.random.default_rng(5 * N + hop + int(int16))
    win = O.sqrt_hann(N)
    kinds, noisy, clean, X64, S64 = [], [], [], [], []
    for i, n in enumerate(lens):
        kind = _kinds(hop).get(n)
        if kind is None:
            continue
        c = pcm[i, :n]
        if kind == "negated":
            x = -c
        elif kind == "same":
            x = c.copy()
        else:
            x = c + _noise(rng, n, int16)
            if kind == "longer":
                x = np.concatenate([x, _noise(rng, 2 * hop + 44, int16)])
            elif kind == "zeros":
                x[1000:1000 + N + hop + 5] = 0
            elif kind == "early":
                x = x[:(-(-n // hop) - 1) * hop + 1]
                assert len(x) < n
        assert x.dtype == c.dtype and R.frames(len(x), N, hop) >= R.frames(n, N, hop)
        nf = R.frames(n, N, hop)
        assert spectra[i].shape == (N // 2 + 1, nf)
        kinds.append(kind)
        noisy.append(R._frozen(x))
        clean.append(c)
        S64.append(spectra[i])
        X64.append(R._frozen(O.stft_mc(R.as_float(x), N, hop, win)[:, :nf].copy()))
    assert sorted(kinds) == sorted(_kinds(hop).values()), kinds
    assert max(R.frames(len(c), N, hop) for c in clean) > MAXLEN
    return tuple(kinds), tuple(noisy), tuple(clean), tuple(X64), tuple(S64)
