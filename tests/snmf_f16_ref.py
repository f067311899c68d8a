"""Shared by tests/test_snmf_f16_host.py and tests/test_gpu_snmf_f16.py: an fp64 emulation of the sparse-NMF
baseline's inference on fp16 matrix-core operands (csrc/snmf_f16.hip, include/drnmf_snmf_f16.h).  It rounds exactly
the operands the kernel rounds, after the per-row power-of-two scale -- the dictionary Wn, the H entering
Lambda = max(H Wn^T, flr), and Lambda entering den = Lambda Wn -- and computes everything else in fp64: the numerator,
the sums, the floor, the update of the master H, the final mask from the master H and the float32 dictionary.

As in the kernel, the first iteration's products take t0 h_init and t0 flr with h_init's own scale
t0 = row_scale(max h_init), and their denominator is multiplied by s / t0 afterwards: s h_init can leave fp16's range
for a silent frame, t0 h_init cannot.

Built on snmf_model_ref's problems and cases; results are computed once per case and kept (callers must not modify
them)."""
import functools

import numpy as np

import snmf_model_ref as R

FLR = 1e-9
# the cases of tests/test_gpu_snmf_f16.py: snmf_model_ref's four and the first shape of the kernel's wide instance
CASES = R.CASES[:3] + [(1, 3, 40, 258)] + R.CASES[3:]
# Bounds of the GPU tests, absolute, max over the elements of a mask (masks lie in [0, 1]): 4 x the worst figure
# measured on the MI355X over every case of tests/test_gpu_snmf_f16.py (its header and DESIGN.md section 6h list
# them).  device - emulation: worst at (1, 17, 33, 48); device - fp64 oracle: worst at 200 iterations.
MEASURED_EMU, MEASURED_EXACT = 6.489e-05, 1.162e-03
TOL_EMU, TOL_EXACT = 4 * MEASURED_EMU, 4 * MEASURED_EXACT
# the "live" case: the emulation must be at least 4 x TOL_EMU from the fp64 oracle, so that a float32 run cannot pass
# for a float16 one.  Of the shapes above only the reference's own 200 iterations at the shipped N get there (1.16e-3
# against 1.04e-3; at 30 iterations the distances are 3.6e-5 .. 1.0e-3: test_snmf_f16_host.py prints them).
LIVE, LIVE_ITER = (3, 7, 129, 200), 200
LIVE_MIN_DISTANCE = 4 * TOL_EMU


# frames masked on top of snmf_model_ref.valid_frames, so that every case with more than one row carries masked rows:
# at (1, 17, ..) row 16 is the second tile's only row -- a row tile that is masked entirely
EXTRA_MASKED = {(1, 17, 33, 48): [(0, 3), (0, 16)], (1, 3, 40, 258): [(0, 1)]}


def valid_frames(B, T, F, N):
    v = R.valid_frames(B, T).copy()
    for b, t in EXTRA_MASKED.get((B, T, F, N), []):
        v[b, t] = False
    return v


@functools.lru_cache(maxsize=None)
def problem(B, T, F, N):
    """snmf_model_ref.problem with the frames of EXTRA_MASKED masked as well."""
    x, W, h_init = R.problem(B, T, F, N)
    x = x.copy()
    x[~valid_frames(B, T, F, N)] = R.MASK_VALUE
    x.setflags(write=False)
    return x, W, h_init


@functools.lru_cache(maxsize=None)
def case_reference(B, T, F, N, n_iter=R.N_ITER, power=1.0):
    """The fp64 oracle (oracle.mu_infer + oracle.snmf_irm through snmf_model_ref.reference_mask) on `problem`."""
    x, W, h_init = problem(B, T, F, N)
    ref = R.reference_mask(x, W, h_init, R.SPARSITY, n_iter, power=power)
    ref.setflags(write=False)
    return ref


F16_MAX = 65504.0
SCALE_E_MIN, SCALE_E_MAX = -40, 100         # csrc/snmf_f16.hip: the clamp of a scale's exponent


def f16(a):
    """Round to nearest even to IEEE half (subnormals kept), back in float64.  Values beyond fp16's largest finite
    number SATURATE there, as the kernel's H and Lambda operands do (the dictionary's entries are at most 1): no
    operand is ever inf, so the zero bins and atoms that pad a chunk in the kernel contribute exact zeros and need
    no counterpart here (test_snmf_f16_host.py runs the emulation with zero bins appended all the same)."""
    return np.minimum(np.asarray(a, np.float64), F16_MAX).astype(np.float16).astype(np.float64)


def row_scale(vmax):
    """s = 2^-e, e = ceil(log2(vmax)) clamped to [SCALE_E_MIN, SCALE_E_MAX], for each entry of vmax (float32
    values); 1 where vmax is 0 (or not finite).  s <= 2^40 keeps the scaled floor s 1e-9 finite in fp16."""
    vmax = np.asarray(vmax, np.float32)
    s = np.ones(vmax.shape, np.float64)
    ok = (vmax > 0) & np.isfinite(vmax)
    fr, e = np.frexp(vmax[ok].astype(np.float64))          # vmax = fr 2^e, fr in [1/2, 1)
    e = np.clip(np.where(fr == 0.5, e - 1, e), SCALE_E_MIN, SCALE_E_MAX)
    s[ok] = np.ldexp(1.0, -e)
    return s


def emulate_mask(x, Wn, hn, sparsity, n_iter, power=1.0, round_operands=True, row_scaled=True):
    """x [B,T,F] float32, Wn [F,N] float32 with unit-norm columns, hn [N] float32 in Wn's basis (what the C entry
    takes: snmf_model_ref.normalised) -> mask [B,T,F] float64, masked frames 0.  round_operands=False: the same
    arithmetic without the three roundings (the scaled iteration in plain fp64).  row_scaled=False: every scale is 1
    -- what a kernel WITHOUT the per-row scale would compute (the tests show that they would notice)."""
    rnd = f16 if round_operands else (lambda a: np.asarray(a, np.float64))
    B, T, F = x.shape
    N = Wn.shape[1]
    valid = np.any(x != np.float32(R.MASK_VALUE), axis=-1)
    out = np.zeros((B, T, F))
    if not valid.any():
        return out
    xv = x[valid]
    V32 = xv if power == 1.0 else (xv * xv if power == 2.0 else np.power(xv, np.float32(power)))   # as the kernel
    s = row_scale(V32.max(axis=1))[:, None]                 # (n, 1)
    if not row_scaled:
        s = np.ones_like(s)
    V = V32.astype(np.float64) * s
    W = Wn.astype(np.float64)
    W16 = rnd(Wn)
    sp, fl = s * float(np.float32(sparsity)), s * float(np.float32(FLR))
    num = V @ W                                             # (n, N)
    H = s * hn.astype(np.float64)[None, :]
    for it in range(int(n_iter)):
        if it == 0:
            t0 = float(row_scale(hn.max())) if row_scaled else 1.0
            A = np.repeat(rnd(t0 * hn.astype(np.float64))[None, :], V.shape[0], axis=0)
            lam = rnd(np.maximum(A @ W16.T, t0 * float(np.float32(FLR))))
            den = (s / t0) * (lam @ W16)
        else:
            lam = rnd(np.maximum(rnd(H) @ W16.T, fl))
            den = lam @ W16
        H = H * num / np.maximum(den + sp, fl)
    r = N // 2
    c = H[:, :r] @ W[:, :r].T
    n = H[:, r:] @ W[:, r:].T
    out[valid] = c / (float(np.float32(FLR)) * s + c + n)
    return out


@functools.lru_cache(maxsize=None)
def case_emulation(B, T, F, N, n_iter=R.N_ITER, power=1.0):
    x, W, h_init = problem(B, T, F, N)
    Wn, hn = R.normalised(W, h_init)
    out = emulate_mask(x, Wn, hn, R.SPARSITY, n_iter, power=power)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def range_problem():
    """x [1,16,129] of the LIVE shape's dictionary, one 16-row tile: row 0 an ordinary frame, 1 the same x 1e-6, 2
    the same x 1e4, 3 all zero but not masked, 4 the same frame with single bins zeroed, 5 masked, 6 the same x 1e-16
    and 7 x 1e-30 (below 2^-40, where the scale's exponent is clamped and the scaled floor is at its largest), 8..
    ordinary frames.  Returns (x, W, h_init)."""
    B, T, F, N = LIVE
    x0, W, h_init = problem(B, T, F, N)
    frames = x0[valid_frames(B, T, F, N)]
    x = np.empty((1, 16, F), np.float32)
    for i in range(16):
        x[0, i] = frames[i % len(frames)]
    x[0, 1] = x[0, 0] * np.float32(1e-6)
    x[0, 2] = x[0, 0] * np.float32(1e4)
    x[0, 3] = 0.0
    x[0, 4] = x[0, 0]
    x[0, 4, [0, 7, 64, 128]] = 0.0
    x[0, 5] = R.MASK_VALUE
    x[0, 6] = x[0, 0] * np.float32(1e-16)
    x[0, 7] = x[0, 0] * np.float32(1e-30)
    x.setflags(write=False)
    return x, W, h_init


RANGE_ROWS = ["ordinary", "x 1e-6", "x 1e4", "all zero", "single zero bins", "masked", "x 1e-16", "x 1e-30"]


@functools.lru_cache(maxsize=None)
def range_references():
    """(emulation, oracle) of range_problem, [1,16,129] each."""
    x, W, h_init = range_problem()
    Wn, hn = R.normalised(W, h_init)
    emu = emulate_mask(x, Wn, hn, R.SPARSITY, R.N_ITER)
    ref = R.reference_mask(x, W, h_init, R.SPARSITY, R.N_ITER)
    for a in (emu, ref):
        a.setflags(write=False)
    return emu, ref


# The LIVE problem times 2^k -- x, sparsity and h_init alike, so the frames stay as alive as they are at k = 0 (with
# the sparsity left at 0.1 a quiet frame's H just goes to 0, whatever the kernel does).  2^-20: without the per-row
# scale Lambda (1e-9 .. 1e-5) would lie in fp16's subnormals; 2^14: x reaches 1e5 and Lambda would overflow fp16.
SCALED_K = [-20, 14]


@functools.lru_cache(maxsize=None)
def scaled_problem(k):
    """(x, W, h_init, sparsity) of LIVE times 2^k (masked frames stay masked)."""
    x, W, h_init = problem(*LIVE)
    f = np.float32(2.0 ** k)
    xs = np.where(x == np.float32(R.MASK_VALUE), x, x * f).astype(np.float32)
    hs = (h_init * f).astype(np.float32)
    for a in (xs, hs):
        a.setflags(write=False)
    return xs, W, hs, R.SPARSITY * float(f)


@functools.lru_cache(maxsize=None)
def scaled_references(k, row_scaled=True):
    """(emulation, oracle) of scaled_problem(k)."""
    x, W, h_init, sp = scaled_problem(k)
    Wn, hn = R.normalised(W, h_init)
    emu = emulate_mask(x, Wn, hn, sp, R.N_ITER, row_scaled=row_scaled)
    ref = R.reference_mask(x, W, h_init, sp, R.N_ITER)
    for a in (emu, ref):
        a.setflags(write=False)
    return emu, ref
