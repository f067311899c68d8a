/*
 * drnmf_snmf_online.h -- C ABI of the online noise-adaptive sparse-NMF baseline in libdrnmf.so: the batch mode of
 * drnmf_snmf_adapt.h turned into its online form on sufficient statistics, so that a row can be fed a few frames at
 * a time.  Every batch row is a stream of its own and carries, in a caller-owned state,
 *     W [F][N]        its dictionary, Wn at reset; the leading n0 atoms stay fixed
 *     A [N][N - n0]   sum of H^T H_upd        Bm [F][N - n0]   sum of V^T H_upd      (0 at reset)
 *     count           the valid frames it has seen (int64)
 *     the frames of its unfinished block: V [block][F] and H [block][N].
 * The i-th valid frame of a row (i counted from the reset) belongs to block k = i / block and lands in slot
 * i % block.  With W(k) the row's dictionary when block k starts:
 *     H_i    = n_iter updates  H <- H * (V_i W) / max(max(H W^T, flr) W + sparsity, flr)  from h_init, W = W(k)
 *     mask_i = Wc Hc / (1e-9 + Wc Hc + Wn Hn),  Wc / Wn the first / last N/2 atoms of W(k)
 * and when the last frame of block k has been processed, in this order,
 *     A  <- forget * A  + H_blk^T H_blk[:, n0:]        Bm <- forget * Bm + V_blk^T H_blk[:, n0:]
 *     w_iter times:  num = Bm,  den = W A  (all columns of W from the iteration before),
 *         W_upd <- W_upd * (num + sum(den * W_upd) W_upd) / max(den + sum(num * W_upd) W_upd, flr),  unit norm restored
 * (for beta == 2, sparse_nmf_gpu.m:232-264 needs V^T H_upd and Lambda^T H_upd = W (H^T H_upd) only).  As in the batch
 * mode the n0 fixed columns are never written and a column whose new norm is 0 or not finite keeps its value.  Masked
 * frames (all F bins equal mask_value) are skipped, not counted, and get a zero mask and zero H_out.  A block that
 * never fills causes no update.
 *
 * A frame's result depends on the row's earlier frames only, and every sum over frames is taken in slot order: one
 * call over a whole row and any sequence of calls over its pieces leave the same bits in mask_out, H_out and the
 * state, whatever B, the padded T, the row's position and the rows beside it.
 *
 * Conventions as in drnmf_snmf_adapt.h: device pointers, caller-owned state and workspace (256-byte aligned), the
 * caller's stream, the handle's mutex, never a synchronisation, status codes, drnmf_last_error; arguments are
 * checked before a device is touched.  Exact fp32 arithmetic: the handle's matrix mode does not apply.
 */
#ifndef DRNMF_SNMF_ONLINE_H
#define DRNMF_SNMF_ONLINE_H

#include "drnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if the kernels take the shape: beta == 2, N even, 2 <= N <= 512, block a multiple of 16 in 16..256; else 0. */
int32_t drnmf_snmf_online_admitted(int32_t F, int32_t N, float beta, int32_t block);

/* Bytes of the state of B rows (a multiple of 256); 0 for a shape the entry points refuse. */
size_t drnmf_snmf_online_state_bytes(int32_t B, int32_t F, int32_t N, int32_t n0, int32_t block);

/* Bytes of workspace of a forward call of B rows of T frames (validity, positions, the block's mask staging, the
 * column pass's buffers); 0 for a shape the entry point refuses.  Nothing in it outlives the call. */
size_t drnmf_snmf_online_workspace_bytes(int32_t B, int32_t T, int32_t F, int32_t N, int32_t n0, int32_t block);

/* W = Wn [F][N] (unit-norm columns), statistics, count and block buffers 0 -- for every row, or with rows [B]
 * (int32 on the device, may be NULL) for the rows whose entry is not 0: one stream of several starts over. */
int32_t drnmf_snmf_online_reset(drnmf_handle_t h, int32_t B, int32_t F, int32_t N, int32_t n0, int32_t block,
                                const float* Wn, const int32_t* rows, void* state, size_t state_bytes, void* stream);

/* x [B][T][F]: the next T frames of every row (masked frames where a row has fewer); h_init [N] in the dictionary's
 * basis; mask_out [B][T][F]; H_out [B][T][N] or NULL.  n_iter >= 0 (0: the mask of h_init), w_iter >= 0 (0: the
 * dictionaries never move), 0 < forget <= 1, 0 <= n0 <= N (n0 = N: the fixed baseline of drnmf_snmf.h up to the order
 * of the sums).  A bad argument returns DRNMF_ERR_INVALID_ARG, a shape drnmf_snmf_online_admitted refuses
 * DRNMF_ERR_UNSUPPORTED, a state or workspace that is NULL, misaligned or short DRNMF_ERR_WORKSPACE.  The number of
 * launches depends on T and block alone: 2 + ((T + 2 block - 2) / block) (4 + 2 w_iter), with n0 == N
 * 2 + 3 ((T + 2 block - 2) / block). */
int32_t drnmf_snmf_online_forward(drnmf_handle_t h, int32_t B, int32_t T, int32_t F, int32_t N, int32_t n0,
                                  int32_t block, int32_t n_iter, int32_t w_iter, float sparsity, float forget,
                                  float power, float mask_value, int32_t has_mask, const float* x,
                                  const float* h_init, float* mask_out, float* H_out, void* state,
                                  size_t state_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* Copies out of the state, each destination optional (NULL): W_out [B][F][N], counts_out [B] (int64), A_out
 * [B][N][N - n0], Bm_out [B][F][N - n0]. */
int32_t drnmf_snmf_online_read(drnmf_handle_t h, int32_t B, int32_t F, int32_t N, int32_t n0, int32_t block,
                               const void* state, size_t state_bytes, float* W_out, int64_t* counts_out,
                               float* A_out, float* Bm_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_SNMF_ONLINE_H */
