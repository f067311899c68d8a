"""Shared by tests/test_snmf_kl_host.py and tests/test_gpu_snmf_kl.py: the cases of the sparse-NMF baseline's
inference under the KL cost (csrc/snmf_kl.hip, include/drnmf_snmf_kl.h), inputs that hold zero bins, and their fp64
references -- snmf_model_ref.reference_mask at beta = 1 for the reference's per-call floor, the same on an input whose
zeros are replaced for a fixed floor.  Built on snmf_model_ref's problems; results are computed once per case and
kept (callers must not modify them).

The bound is the project's mask bound, snmf_model_ref.MASK_MSE_TOL = 1e-8: a float32 restatement of the update
(`restate_mask32`, numpy) lies 6e-15 .. 4e-14 (mask MSE, 30 iterations; 1.3e-13 .. 5.5e-13 at 200) from the fp64
oracle on the four cases of snmf_model_ref, with and without zero bins, while ignoring the floor moves the mask by
3e-5 .. 5e-3 on the inputs with zeros -- test_snmf_kl_host.py prints and checks both sides."""
import functools

import numpy as np

import snmf_model_ref as R

FLR = 1e-9
V_FLOOR = 1e-3               # the fixed floor of the tests
# snmf_model_ref's four and the two sides of the kernel's narrow / wide instance split: np16(N) = 256 and 272.  258 is
# wide with scalar dictionary loads (N % 4 != 0); (1, 1, 5, 10) is narrow with them
CASES = R.CASES + [(1, 2, 40, 256), (1, 3, 33, 258)]
ZERO_FRAME = {(3, 7): (0, 3)}            # (B, T) -> a valid frame that is zero in every bin


@functools.lru_cache(maxsize=None)
def zero_problem(B, T, F, N):
    """snmf_model_ref.problem with zero bins in the valid frames (a fifth of them, RandomState(7)); on the (3, 7, ..)
    case one valid frame is zero in every bin (it stays valid: a masked frame holds MASK_VALUE)."""
    x, W, h_init = R.problem(B, T, F, N)
    x = x.copy()
    valid = np.any(x != np.float32(R.MASK_VALUE), axis=-1)
    z = (np.random.RandomState(7).rand(*x.shape) < 0.2) & valid[..., None]
    x[z] = 0.0
    if (B, T) in ZERO_FRAME:
        b, t = ZERO_FRAME[(B, T)]
        assert valid[b, t]
        x[b, t] = 0.0
    x.setflags(write=False)
    return x, W, h_init


def valid_of(x):
    return np.any(x != np.float32(R.MASK_VALUE), axis=-1)


def substituted(x, v_floor, power=1.0):
    """x with the zeros of its valid frames replaced so that V = x^power holds v_floor there."""
    out = x.copy()
    out[(x == 0) & valid_of(x)[..., None]] = np.float32(v_floor) ** (1.0 / power)
    return out


@functools.lru_cache(maxsize=None)
def case_reference(B, T, F, N, zeros=False, v_floor=None, n_iter=R.N_ITER, power=1.0):
    """fp64 oracle at beta = 1.  v_floor None: the reference's rule (zeros of V raised to the smallest positive entry of
    the valid frames run together); else zeros raised to v_floor."""
    x, W, h_init = zero_problem(B, T, F, N) if zeros else R.problem(B, T, F, N)
    if v_floor is not None:
        x = substituted(x, v_floor, power)
    ref = R.reference_mask(x, W, h_init, R.SPARSITY, n_iter, beta=1.0, power=power)
    ref.setflags(write=False)
    return ref


def restate_mask32(x, Wn, hn, sparsity, n_iter, v_floor=None, use_floor=True):
    """The update as the kernel states it, in numpy float32: x [B,T,F], Wn / hn as the C entry takes them
    (snmf_model_ref.normalised) -> mask [B,T,F] float32.  use_floor=False: zeros of V stay zeros."""
    f32 = np.float32
    valid = valid_of(x)
    out = np.zeros(x.shape, f32)
    V = x[valid].astype(f32)
    if use_floor and V.size and (V > 0).any():
        V = np.where(V == 0, f32(V[V > 0].min() if v_floor is None else v_floor), V)
    H = np.repeat(hn.astype(f32)[None, :], V.shape[0], axis=0)
    den = np.maximum(Wn.sum(axis=0, dtype=f32) + f32(sparsity), f32(FLR))
    for _ in range(int(n_iter)):
        lam = np.maximum(H @ Wn.T, f32(FLR))
        H = H * ((V / lam) @ Wn) / den
    r = Wn.shape[1] // 2
    c, n = H[:, :r] @ Wn[:, :r].T, H[:, r:] @ Wn[:, r:].T
    out[valid] = c / (f32(FLR) + c + n)
    return out
