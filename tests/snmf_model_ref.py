"""Shared by tests/test_snmf_model_host.py and tests/test_gpu_snmf_model.py: the cases of the sparse-NMF baseline's
inference and their fp64 reference -- oracle.mu_infer + oracle.snmf_irm applied to the valid frames with ONE shared
initial vector, masked frames 0.  Computed once per case and kept (lru_cache); callers must not modify it."""
import functools

import numpy as np

from oracle import drnmf_oracle as O

MASK_VALUE = -1.0
MASK_MSE_TOL = 1e-8          # the project's bound for a mask against the oracle (tests/test_gpu_parity.py)
N_ITER, SPARSITY = 30, 0.1

# (B, T, F, N) -> which frames are valid.  What each reaches: see tests/test_gpu_snmf_model.py.
CASES = [(1, 1, 5, 10), (1, 17, 33, 48), (3, 7, 129, 200), (2, 9, 257, 512)]
# shapes outside the tile kernel's admission (N = 514; beta = 1 runs at (3, 7, 129, 200))
WIDE = (1, 17, 33, 514)


def valid_frames(B, T):
    """[B, T] bool.  (3, 7): ragged lengths 7, 4, 0 -- the last sequence is all masked and 16-row tiles straddle
    the sequences.  (2, 9): masked frames in the interior.  Else: every frame."""
    v = np.ones((B, T), dtype=bool)
    if (B, T) == (3, 7):
        v[1, 4:] = False
        v[2, :] = False
    elif (B, T) == (2, 9):
        v[0, [2, 5]] = False
        v[1, [0, 8]] = False
    return v


@functools.lru_cache(maxsize=None)
def problem(B, T, F, N):
    """x [B,T,F] float32 (valid frames: a sparse non-negative mixture of the atoms plus a little noise, strictly
    positive; masked frames: MASK_VALUE in every bin), W [F,N] float32 positive, h_init [N] float32."""
    rng = np.random.RandomState(1000 * F + N)
    # atoms are bumps along the bins, speech atoms centred in the lower part of the band and noise atoms in the
    # upper part (overlapping in the middle): the mask then runs from near 1 to near 0 across a frame
    r = N // 2
    centre = np.concatenate([np.linspace(0, 0.55 * (F - 1), r), np.linspace(0.45 * (F - 1), F - 1, r)])
    bump = np.exp(-((np.arange(F)[:, None] - centre[None, :]) / max(1.0, F / 10.0)) ** 2)
    W = (bump * (0.5 + rng.rand(F, N)) + 0.02 * rng.rand(F, N)).astype(np.float32)
    Ht = rng.rand(B, T, N) * (rng.rand(B, T, N) < max(0.15, 4.0 / N))
    Ht[..., :N // 2] *= rng.rand(B, T, 1) * 2          # frames differ in how much speech they hold
    x = (Ht @ W.T.astype(np.float64) + 0.01 * rng.rand(B, T, F) + 1e-3).astype(np.float32)
    x[~valid_frames(B, T)] = MASK_VALUE
    h_init = rng.rand(N).astype(np.float32)
    for a in (x, W, h_init):
        a.setflags(write=False)
    return x, W, h_init


def reference_mask(x, W, h_init, sparsity, n_iter, beta=2.0, power=1.0):
    """fp64: masks of the valid frames of x [B,T,F] run TOGETHER through mu_infer / snmf_irm, zeros elsewhere."""
    B, T, F = x.shape
    valid = np.any(x != np.float32(MASK_VALUE), axis=-1)
    out = np.zeros((B, T, F))
    if valid.any():
        V = (x[valid].astype(np.float64) ** power).T                     # (F, n)
        H0 = np.repeat(h_init.astype(np.float64)[:, None], V.shape[1], axis=1)
        H, Wn = O.mu_infer(V, W.astype(np.float64), H0, sparsity, n_iter, beta=beta)
        out[valid] = O.snmf_irm(Wn, H, W.shape[1] // 2).T
    return out


@functools.lru_cache(maxsize=None)
def case_reference(B, T, F, N, n_iter=N_ITER, beta=2.0, power=1.0):
    x, W, h_init = problem(B, T, F, N)
    ref = reference_mask(x, W, h_init, SPARSITY, n_iter, beta=beta, power=power)
    ref.setflags(write=False)
    return ref


def normalised(W, h_init):
    """What the C entry takes: (Wn with unit-norm columns, h_init in Wn's basis), float32."""
    nrm = np.sqrt((W.astype(np.float64) ** 2).sum(axis=0))
    return (W / nrm).astype(np.float32), (h_init * nrm).astype(np.float32)
