"""The (N, hop) grid of the transform tests at hops other than N/4, and what both of its test files share
(test_stft_hops_host.py on the CPU, test_gpu_stft_hops.py on the MI355X): the branch every size is meant to take in
csrc/stft.hip, the lengths per size, the batches, and the oracle's spectra and reconstructions, computed once per
size and never modified.  numpy and the oracle only: no GPU needed.

Branches (csrc/stft.hip):
  forward  'fast'      N = 512 / 1024: stft_real_frame, one wave per frame, a Stockham transform of N/2 points
           'general'   every other size: stft_frame, one workgroup per frame, fft_lds (radix 2, with its separate
                       first stage when log2 N is odd)
  inverse  'fused'     N = 512 / 1024 and hop <= N: istft_real_ragged_kernel, a workgroup per run of
                       (2048 // hop) * hop samples
           'two-stage' everything else: istft_frames_ragged_kernel (istft_frame -> fft_lds) into a frames buffer,
                       then overlap_add_ragged_kernel
"""
import functools

import numpy as np

from oracle import drnmf_oracle as O

# (N, hop): (forward, ragged inverse, what the size adds)
GRID = {
    (512, 256): ("fast", "fused", "the default hop, two frames per sample"),
    (1024, 512): ("fast", "fused", "the default hop, two frames per sample"),
    (512, 512): ("fast", "fused", "one frame per sample"),
    (512, 160): ("fast", "fused", "run = 1920, hop does not divide N, nout = k hop - 32"),
    (512, 129): ("fast", "fused", "odd hop: the load path alternates frame by frame"),
    (512, 8): ("fast", "fused", "64 frames per sample; lengths capped at 3000"),
    (1024, 1000): ("fast", "fused", "run = 2000, C = 2"),
    (512, 600): ("fast", "two-stage", "hop > N: uncovered samples are zero; odd log2 N in fft_lds"),
    (1024, 1025): ("fast", "two-stage", "hop > N: uncovered samples are zero"),
    (128, 32): ("general", "two-stage", "odd log2 N"),
    (128, 64): ("general", "two-stage", "odd log2 N, the default hop"),
    (2048, 512): ("general", "two-stage", "odd log2 N, 24 KB LDS"),
    (4096, 1024): ("general", "two-stage", "largest size, 48 KB LDS"),
    (256, 96): ("general", "two-stage", "hop does not divide N"),
    (64, 64): ("general", "two-stage", "hop = N at the smallest size"),
    (64, 100): ("general", "two-stage", "hop > N at the smallest size"),
}
SIZES = list(GRID)
FUSED = [s for s in SIZES if GRID[s][1] == "fused"]
HOP_ABOVE_N = [s for s in SIZES if s[1] > s[0]]
DIVIDING = [s for s in SIZES if s[0] % s[1] == 0]

# the reduced sets of the issue
INDEPENDENCE_SIZES = [(512, 160), (512, 129), (1024, 1000), (512, 600), (128, 64), (256, 96)]
T_CUT_SIZES = [(512, 160), (128, 32)]
PAIR_SIZES = [(512, 256), (512, 160), (128, 64), (2048, 512)]
STREAM_SIZES = [(512, 256), (512, 64), (1024, 512), (128, 32), (2048, 512), (64, 64)]

# the project's bounds (tests/test_gpu_enhance.py): spectrum within 2e-5 max|S|, samples within 1e-4 max|ref|
TOL_FWD, TOL_INV = 2e-5, 1e-4


def ids(sizes):
    return ["%dx%d" % s for s in sizes]


def lengths(N, hop):
    """[1, hop-1, hop, hop+1, 3 hop + 7, 9999, 16001] without the lengths below 1; at most 3000 for (512, 8), whose
    64 frames per sample would otherwise cost seconds on the host; 2 * 4096 + 5 in place of the two long ones for
    (4096, 1024)."""
    lens = [1, hop - 1, hop, hop + 1, 3 * hop + 7, 9999, 16001]
    if (N, hop) == (4096, 1024):
        lens = lens[:5] + [2 * 4096 + 5]
    if (N, hop) == (512, 8):
        lens = [min(n, 3000) for n in lens]
    out = []
    for n in lens:
        if n >= 1 and n not in out:
            out.append(n)
    return out


def equal_lengths(N, hop):
    """The nsampl of the batched entry points: 3 hop + 7 and 9999 (under the caps of `lengths`)."""
    cap = max(lengths(N, hop))
    out = []
    for n in (3 * hop + 7, min(9999, cap)):
        if n not in out:
            out.append(n)
    return out


def frames(n, N, hop):
    """drnmf_stft_frames in closed form: ceil(n / hop) + N // hop + 1."""
    return -(-n // hop) + N // hop + 1


def out_length(n, N, hop, crop=False):
    """hop (frames - 1) - N = ceil(n / hop) hop - (N mod hop) for hop <= N: NOT a multiple of the hop where the
    hop does not divide N."""
    full = hop * (frames(n, N, hop) - 1) - N
    return min(full, n) if crop else full


def fused_run(hop):
    """Samples a workgroup of the fused inverse owns (ragged_run in csrc/stft.hip)."""
    return max(2048 // hop, 1) * hop


def batch(lens, seed, int16, stride=None):
    """As test_gpu_enhance._batch: rows of noise, each valid up to its length and followed by junk the kernels must
    not read as signal; the stride is odd."""
    rng = np.random.default_rng(seed)
    stride = stride or (max(lens) + 1 if max(lens) % 2 == 0 else max(lens) + 2)
    assert stride % 2 == 1
    if int16:
        return rng.integers(-20000, 20000, size=(len(lens), stride)).astype(np.int16)
    return (0.3 * rng.standard_normal((len(lens), stride))).astype(np.float32)


def as_float(row):
    return O.wav_int16_to_float(row) if row.dtype == np.int16 else row


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def signals(N, hop, int16):
    """(lens, pcm) of a size: one batch per input type, shared by every test of the size."""
    lens = lengths(N, hop)
    return lens, _frozen(batch(lens, 7 * N + hop + int(int16), int16))


@functools.lru_cache(maxsize=None)
def spectra(N, hop, int16):
    """O.stft_mc of every row of signals(N, hop, int16): a tuple of complex128 [F, n_frames]."""
    lens, pcm = signals(N, hop, int16)
    w = O.sqrt_hann(N)
    return tuple(_frozen(O.stft_mc(as_float(pcm[i, :n]), N, hop, w)) for i, n in enumerate(lens))


@functools.lru_cache(maxsize=None)
def masks(N, hop):
    """One random mask in [0, 1) per row of the size, float32 [n_frames, F]."""
    rng = np.random.default_rng(N * 31 + hop)
    return tuple(_frozen(rng.random((frames(n, N, hop), N // 2 + 1)).astype(np.float32)) for n in lengths(N, hop))


def reconstruct(S, mask, N, hop, nsampl=None, keep_frames=None):
    """O.reconstruct of spectrum S [F, nf] (mask [nf, F] or None); keep_frames: the frames at or behind it are
    zeroed first, which is what an inverse called with T = keep_frames has to compute."""
    re, im = S.real.copy(), S.imag.copy()
    if keep_frames is not None:
        re[:, keep_frames:] = 0.0
        im[:, keep_frames:] = 0.0
    m = None if mask is None else mask.T.astype(np.float64)
    return O.reconstruct(re, im, m, hop, O.sqrt_hann(N), nsampl)


@functools.lru_cache(maxsize=None)
def reconstructions(N, hop, masked):
    """The uncropped O.reconstruct of every float32 row's oracle spectrum (with masks(N, hop) or without a mask);
    the cropped one is its first `length` samples."""
    S = spectra(N, hop, False)
    m = masks(N, hop) if masked else [None] * len(S)
    return tuple(_frozen(reconstruct(S[i], m[i], N, hop)) for i in range(len(S)))


def uncovered(n_out, N, hop):
    """Boolean [n_out]: the samples no frame covers (hop > N): sample s sits at p = s + N of the untrimmed signal
    and frame f covers [f hop, f hop + N)."""
    p = np.arange(n_out) + N
    return p % hop >= N


def host_fft_error(N, hop):
    """The largest error of a float32 host FFT (torch.fft.rfft on the CPU, float32 windowed frames) against the
    oracle over the float32 rows of the size, relative to max|S| of the row: the yardstick for N = 2048 / 4096
    should the device ever exceed the project's bounds there (the only function here that needs torch)."""
    import torch
    lens, pcm = signals(N, hop, False)
    w = O.sqrt_hann(N).astype(np.float32)
    worst = 0.0
    for i, n in enumerate(lens):
        S = spectra(N, hop, False)[i]
        nfram = -(-n // hop)
        x = np.concatenate([np.zeros(N, np.float32), pcm[i, :n], np.zeros(nfram * hop - n + N, np.float32)])
        idx = np.arange(N)[None, :] + hop * np.arange(S.shape[1])[:, None]
        fr = (x[idx] * w[None, :]).astype(np.float32)
        H = torch.fft.rfft(torch.from_numpy(fr), dim=1).numpy()          # float32 in, complex64 out
        assert H.dtype == np.complex64
        if np.max(np.abs(S)) > 0:                             # (a lone sample under the window's zero: S = 0)
            worst = max(worst, float(np.max(np.abs(np.conj(H).T - S)) / np.max(np.abs(S))))
    return worst


def rel_err(got, ref):
    """max|got - ref| / max|ref|; where the reference is all zero (a lone sample under the window's zero, or under
    no frame at all) 0.0 if got is all zero too and inf otherwise."""
    d, scale = float(np.max(np.abs(got - ref))), float(np.max(np.abs(ref)))
    if scale == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / scale
