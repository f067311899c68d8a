"""numpy fp64 restatement of include/drnmf_resample.h: the filter, the offline sum as the header defines it, and a
chunked form that applies the header's finality and history rules literally.  Both forms sum an output's terms in
ascending k through the same function, so the chunked result equals the offline one exactly."""
import math

import numpy as np

MAX_PQ = 640
NZ, BETA = 10, 5.0

# fs_in -> fs_out of the tests, with p / q
RATE_PAIRS = ((48000, 16000, 1, 3), (8000, 16000, 2, 1), (44100, 16000, 160, 441), (16000, 44100, 441, 160),
              (11025, 16000, 640, 441), (16000, 16000, 1, 1))


def rate(fs_in, fs_out):
    """(p, q) = fs_out / fs_in reduced; ValueError as the library refuses."""
    if fs_in <= 0 or fs_out <= 0 or int(fs_in) != fs_in or int(fs_out) != fs_out:
        raise ValueError("rates must be positive whole numbers")
    g = math.gcd(int(fs_in), int(fs_out))
    p, q = int(fs_out) // g, int(fs_in) // g
    if max(p, q) > MAX_PQ:
        raise ValueError("max(p, q) > %d" % MAX_PQ)
    return p, q


def out_len(n, p, q):
    return -(-int(n) * p // q)


def filter_taps(p, q, nz=NZ, beta=BETA):
    """h [L], L = 2 nz max(p, q) + 1, sum h = p."""
    M = max(p, q)
    L = 2 * nz * M + 1
    half = (L - 1) // 2
    h = np.kaiser(L, beta) * np.sinc((np.arange(L) - half) / M) / M
    return p * h / h.sum()


def first_needed(m, p, q, L):
    """The first sample output m meets: max(0, ceil((q m + half - (L - 1)) / p))."""
    return max(0, -(-(q * m + (L - 1) // 2 - (L - 1)) // p))


def last_needed(m, p, q, L):
    """The sample whose arrival makes output m final: floor((q m + half) / p)."""
    return (q * m + (L - 1) // 2) // p


def _outputs(buf, buf_from, n, m, h, p, q):
    """y[m] for the output indices m (int64 array) of a signal of which n samples are known and buf holds
    x[buf_from .. buf_from + len(buf)): per output one chain over ascending k, vectorised over the outputs."""
    L = len(h)
    half = (L - 1) // 2
    m = np.asarray(m, dtype=np.int64)
    acc = np.zeros(m.shape[0], dtype=np.float64)
    if m.shape[0] == 0:
        return acc
    t0 = q * m + half
    k0 = np.maximum(-(-(t0 - (L - 1)) // p), 0)
    k1 = np.minimum(t0 // p, n - 1)
    assert (k0[k1 >= k0] >= buf_from).all(), "the history rule was broken"
    for c in range(max(int((k1 - k0).max()) + 1, 0)):
        k = k0 + c
        ok = k <= k1
        xi = np.where(ok, k - buf_from, 0)
        ti = np.where(ok, t0 - p * k, 0)
        acc = np.where(ok, acc + buf[xi] * h[ti], acc)
    return acc


def as_samples(x):
    """The float64 values of int16 (v / 32768) or float32 samples."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.float64) / 32768.0
    return x.astype(np.float64)


def resample(x, p, q, h=None, nz=NZ, beta=BETA):
    """The offline definition: ceil(n p / q) outputs in fp64 (p == q == 1: the samples themselves)."""
    x = as_samples(x)
    n = x.shape[0]
    if p == 1 and q == 1:
        return x.copy()
    if h is None:
        h = filter_taps(p, q, nz, beta)
    if n == 0:
        return np.zeros(0)
    return _outputs(x, 0, n, np.arange(out_len(n, p, q), dtype=np.int64), h, p, q)


def resample_chunked(x, p, q, cuts, h=None, nz=NZ, beta=BETA, history=None):
    """x fed in the pieces x[cuts[i]:cuts[i + 1]] (cuts ascending from 0 to len(x); equal neighbours are empty
    chunks), then closed.  After every piece the outputs that have become final are computed from the history kept
    and the piece; the history then shrinks to what the next output needs.  Returns the concatenation; `history`
    (a list) collects the samples held after each piece."""
    x = as_samples(x)
    if h is None:
        h = np.ones(1) if p == q == 1 else filter_taps(p, q, nz, beta)
    L = len(h)
    buf, buf_from, n_in, n_out, out = np.zeros(0), 0, 0, 0, []
    pieces = [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    for i, piece in enumerate(pieces + [None]):
        closing = piece is None
        if not closing:
            buf = np.concatenate([buf, piece])
            n_in += piece.shape[0]
        end = n_out
        if closing:
            end = out_len(n_in, p, q)
        else:
            while last_needed(end, p, q, L) <= n_in - 1:
                end += 1
        out.append(_outputs(buf, buf_from, n_in, np.arange(n_out, end, dtype=np.int64), h, p, q))
        n_out = end
        keep_from = min(first_needed(n_out, p, q, L), n_in)
        buf, buf_from = buf[keep_from - buf_from:], keep_from
        if history is not None:
            history.append(buf.shape[0])
    assert n_out == out_len(x.shape[0], p, q)
    return np.concatenate(out)


def chunkings(n, seed, big):
    """The cuts of the tests for a recording of n samples: all one-sample chunks; chunks of 0 interleaved; one chunk
    larger than `big`; a seeded random cut."""
    rs = np.random.RandomState(seed)
    ones = list(range(n + 1))
    zeros = sorted(list(range(0, n + 1, 7)) * 2 + [n, n])
    one_big = [0, min(5, n), min(5 + big + 3, n), n]
    rnd = [0] + sorted(rs.randint(0, n + 1, 9).tolist()) + [n]
    return dict(ones=ones, zeros=zeros, big=one_big, random=rnd)
