"""Numpy reference of the online noise-adaptive sparse-NMF baseline (include/drnmf_snmf_online.h).  Every batch row
is a stream with a state of its own: the dictionary W (Wn at the start), the statistics A [N, N-n0] and Bm [F, N-n0]
(0), the count of valid frames seen, and the V and H of the current unfinished block.

The i-th valid frame of a row belongs to block k = i // L and is decomposed (oracle.mu_infer's H-only updates, beta
= 2, from h_init) and masked (oracle.snmf_irm) with W(k), the dictionary in force when block k starts.  When the
block's last frame has been processed:  A <- rho A + H^T H[:, n0:],  Bm <- rho Bm + V^T H[:, n0:]  over its L frames,
then w_iter times  num = Bm, den = W A,  the column update of sparse_nmf_gpu.m:232-264 and the unit norm; rules 1 and
2 of tests/snmf_adapt_ref.py hold (fixed columns are never written; a column whose new norm is 0 or not finite keeps
its value).  Masked frames are skipped and not counted; a block that never fills causes no update.

The arithmetic runs in `dtype` (float64 by default; the GPU tests also run it in float32 to measure what float32
itself costs)."""
import numpy as np

from snmf_adapt_ref import FLR, irm, valid_frames


class Row(object):
    """The state of one stream."""

    def __init__(self, Wn, n0, L, dtype=np.float64):
        self.W = np.array(Wn, dtype=dtype, copy=True)
        F, N = self.W.shape
        self.n0, self.L, self.dtype = int(n0), int(L), dtype
        self.A = np.zeros((N, N - self.n0), dtype)
        self.Bm = np.zeros((F, N - self.n0), dtype)
        self.count = 0
        self.V, self.H = [], []               # the unfinished block's frames
        self.blocks = []                      # (V_blk, H_blk, the W they were decomposed with) of every finished block


def infer_frame(v, W, h_init, sparsity, n_iter):
    """n_iter H-only updates of one frame v (F,) on W (oracle.mu_infer, beta = 2, in the arithmetic of W's dtype)."""
    dt = W.dtype.type
    flr, sp = dt(FLR), dt(sparsity)
    h = np.array(h_init, dtype=W.dtype, copy=True)
    num = W.T @ v
    for _ in range(int(n_iter)):
        lam = np.maximum(W @ h, flr)
        h = h * num / np.maximum(W.T @ lam + sp, flr)
    return h


def update_w(W, A, Bm, n0, w_iter):
    """w_iter column updates of W[:, n0:] from the statistics; returns the new dictionary."""
    dt = W.dtype.type
    W = W.copy()
    for _ in range(int(w_iter)):
        if n0 >= W.shape[1]:
            break
        Wu = W[:, n0:]
        num, den = Bm, W @ A
        dpw = np.maximum(den + np.sum(num * Wu, 0, keepdims=True) * Wu, dt(FLR))
        dmw = num + np.sum(den * Wu, 0, keepdims=True) * Wu
        with np.errstate(all="ignore"):
            Wnew = Wu * dmw / dpw
            nrm = np.sqrt(np.sum(Wnew * Wnew, axis=0))
            ok = np.isfinite(nrm) & (nrm > 0)                   # rule 2
            cols = n0 + np.where(ok)[0]
            W[:, cols] = Wnew[:, ok] / nrm[ok]                  # rule 1: nothing else is written
    return W


def push_row(row, x_row, h_init, sparsity, n_iter, w_iter=1, forget=1.0, power=1.0, mask_value=-1.0):
    """The next frames x_row (T, F) float32 of one stream -> mask (T, F), H (T, N) in the row's dtype."""
    dt = row.dtype
    x_row = np.asarray(x_row, np.float32)
    T, F = x_row.shape
    N = row.W.shape[1]
    mask, H = np.zeros((T, F), dt), np.zeros((T, N), dt)
    ok = valid_frames(x_row, mask_value)
    for t in range(T):
        if not ok[t]:
            continue
        v = x_row[t].astype(dt) ** dt(power)
        h = infer_frame(v, row.W, h_init, sparsity, n_iter)
        H[t] = h
        mask[t] = irm(row.W, h[None, :], N // 2)[0]
        row.V.append(v)
        row.H.append(h)
        row.count += 1
        if len(row.V) == row.L:
            Vb, Hb = np.stack(row.V), np.stack(row.H)
            row.blocks.append((Vb, Hb, row.W.copy()))
            row.A = dt(forget) * row.A + Hb.T @ Hb[:, row.n0:]
            row.Bm = dt(forget) * row.Bm + Vb.T @ Hb[:, row.n0:]
            row.W = update_w(row.W, row.A, row.Bm, row.n0, w_iter)
            row.V, row.H = [], []
    return mask, H


def online_forward(x, Wn, h_init, sparsity, n_iter, n0, L, w_iter=1, forget=1.0, power=1.0, mask_value=-1.0,
                   dtype=np.float64, rows=None):
    """x (B, T, F) -> mask (B, T, F), H (B, T, N), rows (the list of Row states, continued when given)."""
    x = np.asarray(x, np.float32)
    B, T, F = x.shape
    N = np.asarray(Wn).shape[1]
    if rows is None:
        rows = [Row(Wn, n0, L, dtype) for _ in range(B)]
    mask, H = np.zeros((B, T, F), dtype), np.zeros((B, T, N), dtype)
    for b in range(B):
        mask[b], H[b] = push_row(rows[b], x[b], h_init, sparsity, n_iter, w_iter=w_iter, forget=forget, power=power,
                                 mask_value=mask_value)
    return mask, H, rows


def mixture(B, T, F, N, n0, lengths=None, seed=11, mask_value=-1.0):
    """The synthetic mixtures of the adaptive tests: a speech part from the model's first n0 atoms plus noise from a
    dictionary the model has not seen, 30 % of the activations non-zero; W = rand + 0.05, one shared h_init.
    Returns x (B, T, F) float32 (mask_value behind a row's length), Wn (F, N) float32 with unit-norm columns and
    h_init (N,) float32 in Wn's basis."""
    lengths = lengths or (T,) * B
    rng = np.random.RandomState(seed)
    W = rng.rand(F, N) + 0.05
    D = rng.rand(F, max(N - n0, N // 2)) + 0.05
    h_init = rng.rand(N)
    x = np.full((B, T, F), mask_value, np.float32)
    for b, n in enumerate(lengths):
        Hs = rng.rand(n, n0) * (rng.rand(n, n0) < 0.3)
        Hn = rng.rand(n, D.shape[1]) * (rng.rand(n, D.shape[1]) < 0.3)
        x[b, :n] = Hs @ W[:, :n0].T + Hn @ D.T
    nrm = np.sqrt((W * W).sum(0))
    return x, (W / nrm).astype(np.float32), (h_init * nrm).astype(np.float32)


def divergence(V, W, H):
    """sum (V - W H)^2, V (n, F), W (F, N), H (n, N), in float64."""
    V, W, H = (np.asarray(a, np.float64) for a in (V, W, H))
    return float(np.sum((V - H @ W.T) ** 2))
