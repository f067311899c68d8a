/*
 * drnmf_snmf_kl.h -- C ABI of the sparse-NMF baseline's inference under the Kullback-Leibler cost (the reference's
 * cf 'kl', beta == 1) in libdrnmf.so, as ONE launch per call: what drnmf_snmf.h's tile path is for beta == 2.
 * Padded sequences in, the ratio mask out.  Per valid frame, with the column-normalised dictionary Wn and
 * flr = 1e-9 (sparse_nmf_gpu.m:172, 201-205, 212-216, 228):
 *     V = x^power, zeros raised to the floor (below);  H <- h_init;
 *     den[n] = max(sum_f Wn[f][n] + sparsity, flr)                          (the same for every frame)
 *     n_iter times:  Lambda = max(H Wn^T, flr);  H <- H .* ((V ./ Lambda) Wn) ./ den
 *     mask = Wc Hc / (1e-9 + Wc Hc + Wn Hn),  Wc / Wn the first / last N/2 atoms.
 * A workgroup owns 16 frame rows for all iterations (csrc/snmf_kl.hip); exact-fp32 products, correctly rounded
 * divisions, sums in an order that depends neither on a row's position nor on the rows beside it.
 *
 * The floor.  The reference raises the zeros of V to the smallest positive entry of the CALL's V, so a frame that
 * holds a zero bin depends on the frames it is run with.  v_floor == 0 is that rule (a pass over the valid rows in
 * front of the kernel; a call without a positive entry raises nothing, and the masks of its frames are 0).
 * v_floor > 0 raises zeros to that constant instead: a frame's mask is then a function of that frame, the
 * dictionary and h_init alone, bit for bit, and any split of the rows into calls gives the same bits.  (Without a
 * zero bin in the call the two agree, and the same holds.)
 *
 * Conventions as in drnmf.h: device pointers, caller-owned memory (nothing is allocated inside a call), the
 * caller's stream, the handle's mutex, never a synchronisation, status codes, drnmf_last_error.  Masking as in
 * drnmf_snmf.h: a frame whose F bins ALL equal mask_value is masked and its row of the mask is 0; has_mask = 0:
 * every frame is valid.  The handle's matrix mode plays no part.
 */
#ifndef DRNMF_SNMF_KL_H
#define DRNMF_SNMF_KL_H

#include "drnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if the kernel takes the shape: F > 0 and 2 <= N <= 512; else 0. */
int32_t drnmf_snmf_kl_admitted(int32_t F, int32_t N);

/* Bytes of workspace a call needs (the floor as the kernel reads it); a multiple of 256, whatever the shape. */
size_t drnmf_snmf_kl_workspace_bytes(void);

/* The row count B * T up to which this kernel measured faster than the GEMM path of drnmf_snmf.h at beta == 1
 * (DESIGN.md section 6h); 0: nowhere.  layers.SparseNMFModel's path 'auto' follows it. */
int64_t drnmf_snmf_kl_auto_max_rows(void);

/* x [B][T][F]; Wn [F][N] with unit-norm columns (N even); h_init [N] in Wn's basis; mask_out [B][T][F].
 * power: V = x^power.  n_iter >= 0, sparsity >= 0.  v_floor: 0 or a positive finite constant (see above); negative,
 * NaN or infinite is DRNMF_ERR_INVALID_ARG.  N odd is DRNMF_ERR_INVALID_ARG, N > 512 DRNMF_ERR_UNSUPPORTED.
 * workspace: 4-byte aligned, >= drnmf_snmf_kl_workspace_bytes (else DRNMF_ERR_WORKSPACE), required for either
 * v_floor. */
int32_t drnmf_snmf_kl_forward(drnmf_handle_t h, int32_t B, int32_t T, int32_t F, int32_t N, int32_t n_iter,
                              float sparsity, float power, float mask_value, int32_t has_mask, const float* x,
                              const float* Wn, const float* h_init, float v_floor, float* mask_out, void* workspace,
                              size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_SNMF_KL_H */
