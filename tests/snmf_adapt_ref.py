"""Numpy reference of the noise-adaptive sparse-NMF baseline (include/drnmf_snmf_adapt.h): per batch row, the loop
of oracle.sparse_nmf_train (beta = 2, conv_eps = 0, w_update_ind false on the first n0 atoms) over the row's valid
frames, then oracle.snmf_irm -- with the three rules the project adds to it:

  1. the n0 fixed columns are never written (the oracle divides them by a norm that is 1 up to rounding);
  2. an updated column whose new norm is 0 or not finite keeps the previous iteration's column;
  3. a row without a valid frame leaves its dictionary as Wn and its mask 0; n_iter = 0 gives the mask of h_init
     and Wn.

The arithmetic runs in `dtype` (float64 by default; the GPU tests also run it in float32 to measure what float32
itself costs)."""
import numpy as np

FLR = 1e-9


def valid_frames(x_row, mask_value):
    """keras.layers.Masking: a frame is masked when every bin equals mask_value (None: no frame is masked)."""
    if mask_value is None:
        return np.ones(x_row.shape[0], bool)
    return np.any(x_row != np.float32(mask_value), axis=1)


def adapt_row(V, Wn, h_init, sparsity, n_iter, n0, dtype=np.float64):
    """V (n, F) valid frames of one row, already raised to the power; Wn (F, N); h_init (N,).
    Returns W (F, N), H (n, N) in `dtype`."""
    V = np.asarray(V, dtype)
    W = np.array(Wn, dtype=dtype, copy=True)
    n, N = V.shape[0], W.shape[1]
    H = np.tile(np.asarray(h_init, dtype)[None, :], (n, 1))
    flr, sp = dtype(FLR), dtype(sparsity)
    upd = np.arange(N) >= int(n0)
    if n == 0:
        return W, H
    Vt = V.T                                                    # the oracle's (F, n) layout
    Ht = H.T.copy()
    lam = np.maximum(W @ Ht, flr)
    for _ in range(int(n_iter)):
        dph = np.maximum(W.T @ lam + sp, flr)                   # sparse_nmf_gpu.m:210-229
        dmh = W.T @ Vt
        Ht = Ht * dmh / dph
        lam = np.maximum(W @ Ht, flr)
        if upd.any():                                           # :232-264
            Hw, Ww = Ht[upd], W[:, upd]
            num, den = Vt @ Hw.T, lam @ Hw.T
            dpw = np.maximum(den + np.sum(num * Ww, 0, keepdims=True) * Ww, flr)
            dmw = num + np.sum(den * Ww, 0, keepdims=True) * Ww
            Wnew = Ww * dmw / dpw
            nrm = np.sqrt(np.sum(Wnew * Wnew, axis=0))
            ok = np.isfinite(nrm) & (nrm > 0)                   # rule 2
            cols = np.where(upd)[0]
            W[:, cols[ok]] = Wnew[:, ok] / nrm[ok]              # rule 1: nothing else is written
            lam = np.maximum(W @ Ht, flr)
    return W, Ht.T.copy()


def irm(W, H, r):
    """oracle.snmf_irm in row layout: H (n, N) -> mask (n, F)."""
    c = H[:, :r] @ W[:, :r].T
    n = H[:, r:] @ W[:, r:].T
    return c / (W.dtype.type(1e-9) + c + n)


def adapt_forward(x, Wn, h_init, sparsity, n_iter, n0, power=1.0, mask_value=-1.0, dtype=np.float64):
    """x (B, T, F) -> mask (B, T, F), W (B, F, N), H (B, T, N) in `dtype`; masked frames 0 in mask and H."""
    x = np.asarray(x, np.float32)
    B, T, F = x.shape
    N = Wn.shape[1]
    mask = np.zeros((B, T, F), dtype)
    Wout = np.zeros((B, F, N), dtype)
    Hout = np.zeros((B, T, N), dtype)
    for b in range(B):
        v = valid_frames(x[b], mask_value)
        V = x[b][v].astype(dtype) ** dtype(power)
        W, H = adapt_row(V, Wn, h_init, sparsity, n_iter, n0, dtype=dtype)
        Wout[b] = W
        if v.any():
            Hout[b][v] = H
            mask[b][v] = irm(W, H, N // 2)
    return mask, Wout, Hout


def divergence(V, W, H):
    """sum (V - W H)^2 of one row, V (n, F), W (F, N), H (n, N), in float64."""
    V, W, H = (np.asarray(a, np.float64) for a in (V, W, H))
    return float(np.sum((V - H @ W.T) ** 2))
