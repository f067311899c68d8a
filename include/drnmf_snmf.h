/*
 * drnmf_snmf.h -- C ABI of the sparse-NMF baseline's inference in libdrnmf.so: the reference's third model
 * branch (model == 'snmf', enhance.py:838-852), padded sequences in, the ratio mask out.  Per valid frame:
 *     V = x^power;  H <- h_init;  n_iter multiplicative updates of H with the dictionary fixed
 *     (sparse_nmf_gpu.m:210-229);  mask = Wc Hc / (1e-9 + Wc Hc + Wn Hn),  Wc / Wn the first / last N/2 atoms.
 * Conventions as in drnmf.h: device pointers, caller-owned memory (nothing is allocated inside a call), the
 * caller's stream, the handle's mutex, never a synchronisation, status codes, drnmf_last_error.
 *
 * Masking as in the other models (keras.layers.Masking): a frame whose F bins ALL equal mask_value is masked; its
 * row of the mask is 0.  has_mask = 0: every frame is valid.
 *
 * Every frame starts from the same h_init, so for beta == 2 a frame's mask is a function of that frame alone.  On
 * the tile path it is so bit for bit: a row's sums are taken in an order that depends neither on the row's position
 * nor on the rows beside it, so any split of the rows into calls gives the same bits.  For beta != 2 (GEMM path only)
 * it holds for frames without a zero bin: drnmf_mu_forward raises the zeros of V to the smallest positive entry of
 * the CALL's V (sparse_nmf_gpu.m:201-205), so a frame that holds a zero depends on the frames it is run with.
 */
#ifndef DRNMF_SNMF_H
#define DRNMF_SNMF_H

#include "drnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* which kernels a call takes */
enum {
    DRNMF_SNMF_PATH_AUTO = 0, /* the tile kernel when drnmf_snmf_mask_admitted and B * T is at most the row count up
                               * to which it measured faster, else the GEMM path */
    DRNMF_SNMF_PATH_GEMM = 1, /* drnmf_mu_forward's launches: three device-wide products per iteration */
    DRNMF_SNMF_PATH_TILE = 2  /* one launch: a workgroup owns 16 rows for all n_iter iterations;
                               * DRNMF_ERR_UNSUPPORTED when the shape is not admitted */
};

/* 1 if the tile kernel takes the shape: beta == 2 and 2 <= N <= 512 (H and the numerator V Wn of 16 rows stay in
 * registers and LDS, the dictionary is streamed through LDS 32 bins at a time); else 0. */
int32_t drnmf_snmf_mask_admitted(int32_t F, int32_t N, float beta);

/* Bytes of workspace the GEMM path needs for B x T frames (V, H, a dictionary copy, validity flags and
 * drnmf_mu_forward's own workspace); 0 for a shape the entry point refuses.  The tile path needs none. */
size_t drnmf_snmf_mask_workspace_bytes(int32_t B, int32_t T, int32_t F, int32_t N);

/* x [B][T][F]; Wn [F][N] with unit-norm columns, as drnmf_mu_forward writes it (N even); h_init [N], the initial
 * activation of every frame in that normalised basis (an initial value for the raw dictionary times its column
 * norms); mask_out [B][T][F].  power: V = x^power (enhance.py:754-757).  n_iter >= 0, sparsity >= 0.
 * workspace: 256-byte aligned, >= drnmf_snmf_mask_workspace_bytes (else DRNMF_ERR_WORKSPACE) when the GEMM path is
 * taken; not read on the tile path (may be NULL).  The GEMM path computes beta != 2 as drnmf_mu_forward does (zeros
 * of V are raised to the smallest positive entry of the call's V). */
int32_t drnmf_snmf_mask_forward(drnmf_handle_t h, int32_t B, int32_t T, int32_t F, int32_t N, int32_t n_iter,
                                float beta, float sparsity, float power, float mask_value, int32_t has_mask,
                                const float* x, const float* Wn, const float* h_init, float* mask_out,
                                int32_t path, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_SNMF_H */
