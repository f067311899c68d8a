/*
 * drnmf_snmf_adapt.h -- C ABI of the noise-adaptive sparse-NMF baseline in libdrnmf.so: semi-supervised NMF per
 * batch row.  A row (one recording, or one cut of it) keeps the leading n0 atoms of the dictionary fixed and fits
 * the other N - n0 to its own valid frames: sparse-NMF with w_update_ind false on the first n0 atoms
 * (sparse_nmf_gpu.m:210-264, beta == 2; the reference runs it for stage two of dictionary training,
 * enhance.py:110-116).  Per row, with V = x^power over the row's valid frames, n_iter times:
 *     H <- H * (V W) / max(Lambda W + sparsity, flr),  Lambda = max(H W^T, flr)           (:210-229)
 *     num = V^T H_upd,  den = Lambda^T H_upd   over the updated atoms, Lambda from the new H
 *     W_upd <- W_upd * (num + sum(den * W_upd) W_upd) / max(den + sum(num * W_upd) W_upd, flr)   (:232-258)
 *     W_upd <- W_upd / its column norms; H is not rescaled                                  (:262)
 * then mask = Wc Hc / (1e-9 + Wc Hc + Wn Hn), Wc / Wn the first / last N/2 atoms of the row's dictionary.
 *
 * Beyond the Matlab loop: the n0 fixed columns are never written (they leave with the bits of Wn); an updated
 * column whose new norm is 0 or not finite keeps the previous iteration's column (a digitally silent row); a row
 * without a valid frame leaves its dictionary as Wn and its mask 0.  n_iter = 0 gives the mask of h_init and Wn.
 *
 * Conventions as in drnmf_snmf.h: device pointers, caller-owned memory, the caller's stream, the handle's mutex,
 * never a synchronisation, status codes, drnmf_last_error.  Masking as there: a frame whose F bins all equal
 * mask_value is masked.  Every sum over a row's frames is taken in an order fixed by the frame index, so a row's
 * mask, dictionary and activations have the same bits whatever B, the padded T, the row's position and the rows
 * beside it.
 */
#ifndef DRNMF_SNMF_ADAPT_H
#define DRNMF_SNMF_ADAPT_H

#include "drnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if the kernels take the shape: beta == 2 and 2 <= N <= 512 (the tile kernel's rule in drnmf_snmf.h); else 0. */
int32_t drnmf_snmf_adapt_admitted(int32_t F, int32_t N, float beta);

/* Bytes of workspace for B rows of T frames (every row's dictionary and activations, the validity flags and the
 * per-frame-block partial statistics of the N - n0 updated atoms); 0 for a shape the entry point refuses. */
size_t drnmf_snmf_adapt_workspace_bytes(int32_t B, int32_t T, int32_t F, int32_t N, int32_t n0);

/* x [B][T][F]; Wn [F][N] with unit-norm columns (N even); h_init [N] in that basis; mask_out [B][T][F].
 * n0: the number of fixed leading atoms, 0 <= n0 <= N (n0 = N: the fixed baseline of drnmf_snmf.h up to the order of
 * the sums).  W_out [B][F][N] and H_out [B][T][N] (either may be NULL): every row's final dictionary and
 * activations, in the normalised basis; H_out is 0 at masked frames.  workspace: 256-byte aligned, at least
 * drnmf_snmf_adapt_workspace_bytes (else DRNMF_ERR_WORKSPACE).  A shape that drnmf_snmf_adapt_admitted refuses
 * returns DRNMF_ERR_UNSUPPORTED. */
int32_t drnmf_snmf_adapt_forward(drnmf_handle_t h, int32_t B, int32_t T, int32_t F, int32_t N, int32_t n0,
                                 int32_t n_iter, float sparsity, float power, float mask_value, int32_t has_mask,
                                 const float* x, const float* Wn, const float* h_init, float* mask_out,
                                 float* W_out, float* H_out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_SNMF_ADAPT_H */
