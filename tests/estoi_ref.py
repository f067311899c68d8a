"""fp64 numpy restatement of ESTOI -- the contract of drnmf_stoi_ext (include/drnmf_estoi.h) and of
estoi_segment_kernel in csrc/stoi.hip.  No scipy, no GPU.

[ESTOI-memory]: Jensen & Taal, "An Algorithm for Predicting the Intelligibility of Speech Masked by Modulated
Noise Maskers", IEEE/ACM TASLP 24(11), 2016.  The paper's Matlab code is not part of the reference repository;
this is a restatement of the published algorithm.  x = reference (clean), y = estimate.

1-3. stoi_ref.py's: resample to 10 kHz, drop the silent frames of x, band envelopes [nf, 15].
4'.  Segment m = 0 .. nf - 30 holds band frames m .. m + 29 as 15 x 30 matrices X, Y (band by frame).  rc(A):
     subtract every row's mean, divide every row by its norm, subtract every column's mean, divide every column
     by its norm.  d_m = sum(rc(X) * rc(Y)) / 30; ESTOI = mean d_m.
5.   Plain arithmetic, no epsilon and no noise term: fewer than 30 frames -> NaN; a zero norm -> 0 / 0 = NaN,
     which propagates to the mean.
"""
import numpy as np

import stoi_ref as R

N_SEG = R.N_SEG
J = R.J


def rc(A):
    """Row then column normalisation of a [15, 30] segment."""
    with np.errstate(divide="ignore", invalid="ignore"):
        A = A - A.mean(axis=1, keepdims=True)
        A = A / np.sqrt((A * A).sum(axis=1, keepdims=True))
        A = A - A.mean(axis=0, keepdims=True)
        A = A / np.sqrt((A * A).sum(axis=0, keepdims=True))
    return A


def segment_scores(env_x, env_y):
    """d [max(nf - 29, 0)] for the envelopes env_x, env_y [nf, 15]."""
    X = np.asarray(env_x, dtype=np.float64)
    Y = np.asarray(env_y, dtype=np.float64)
    nf = X.shape[0]
    d = np.zeros(max(nf - N_SEG + 1, 0))
    for m in range(len(d)):
        d[m] = (rc(X[m:m + N_SEG].T) * rc(Y[m:m + N_SEG].T)).sum() / N_SEG
    return d


def estoi_from_env(env_x, env_y, return_parts=False):
    """ESTOI of band envelopes [nf, 15] (any float dtype; the arithmetic is fp64)."""
    d = segment_scores(env_x, env_y)
    val = float(d.mean()) if d.size else float("nan")
    if return_parts:
        return val, dict(d_ext=d)
    return val


def estoi(x, y, fs, return_parts=False):
    """ESTOI of estimate y against reference x (1-D arrays at fs), fp64.  The parts are stoi_ref.stoi's plus
    d_ext [nf - 29] and stoi, the STOI of the same envelopes."""
    s, parts = R.stoi(x, y, fs, return_parts=True)
    val, more = estoi_from_env(parts["env_ref"], parts["env_est"], return_parts=True)
    if return_parts:
        parts = dict(parts, stoi=s, **more)
        return val, parts
    return val


ORACLE_SECONDS = (2.6, 3.1, 1.9, 2.2, 2.8, 3.4)
NOISE_DB = (-5, 0, 5, 10)


def batch(fs, seed, lengths):
    """(E, X) float32 [len(lengths), max(lengths)], zero-padded rows: speech-like references X; estimates E = the
    reference plus noise at -5, 0, 5, 10 dB and a low-passed, delayed copy, cycled over the rows."""
    rng = np.random.default_rng(seed)
    E = np.zeros((len(lengths), max(lengths)), np.float32)
    X = np.zeros_like(E)
    for i, n in enumerate(lengths):
        x = R.speech_like(rng, n, fs).astype(np.float32)
        kind = i % 5
        y = R.lowpass_delay(x, 23) if kind == 4 else R.add_noise(rng, x, NOISE_DB[kind])
        X[i, :n], E[i, :n] = x, y.astype(np.float32)
    return E, X


_oracle_cache = {}


def oracle_batch(fs):
    """The six rows the GPU test scores at fs, with the reference's results: (lengths, E, X, want), want[i] =
    (estoi, parts) of row i.  Computed once per process."""
    if fs not in _oracle_cache:
        lengths = [int(fs * s) for s in ORACLE_SECONDS]
        E, X = batch(fs, 10 + fs // 1000, lengths)
        want = [estoi(X[i, :n].astype(np.float64), E[i, :n].astype(np.float64), fs, return_parts=True)
                for i, n in enumerate(lengths)]
        _oracle_cache[fs] = (lengths, E, X, want)
    return _oracle_cache[fs]
