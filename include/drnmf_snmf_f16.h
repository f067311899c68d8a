/*
 * drnmf_snmf_f16.h -- C ABI of the sparse-NMF baseline's inference on fp16 matrix-core operands in libdrnmf.so:
 * what drnmf_snmf.h's tile path computes (padded sequences in, the ratio mask out; beta == 2), with the three
 * operands of the iteration's two products rounded to fp16 and contracted on v_mfma_f32_16x16x32_f16 with fp32
 * accumulation:
 *     the dictionary Wn (packed once: drnmf_snmf_f16_pack_dict), the current H entering Lambda = max(H Wn^T, flr),
 *     and Lambda entering the denominator Lambda Wn.
 * Everything else is fp32: the numerator V Wn (exact fp32 products, once), the denominator's sum, the floor, the
 * update H <- H * num / max(den + sparsity, flr) on an fp32 master copy of H (the fp16 H is a rounded shadow of
 * it), and the two products of the final mask, taken from the fp32 master and the fp32 dictionary.
 *
 * Range.  Every valid frame is scaled by a power of two of its own, s = 2^-e with e = ceil(log2(max_f V[f]))
 * clamped to [-40, 100] (s = 1 for an all-zero frame; the clamp keeps the scaled floor finite in fp16, and the H and
 * Lambda operands saturate at fp16's largest finite value, so no operand is ever inf): V, h_init, sparsity, the floor and the mask's 1e-9 are multiplied by s, which leaves the
 * iteration algebraically as it is and is exact in fp32, and puts V's largest bin into (1/2, 1] whatever the
 * level of the frame.  The first iteration's products take h_init under a scale of its own, t0 = 2^-ceil(log2 max
 * h_init) (s h_init can leave fp16's range for a silent frame), and their denominator is multiplied by s / t0
 * afterwards, again exactly.
 *
 * Conventions as in drnmf.h: device pointers, caller-owned memory (nothing is allocated inside a call), the
 * caller's stream, the handle's mutex, never a synchronisation, status codes, drnmf_last_error.  Masking as in
 * drnmf_snmf.h.  A frame's mask is a function of that frame, the dictionary and h_init alone, bit for bit: any
 * split of the rows into calls gives the same bits.  The handle's matrix mode plays no part.
 */
#ifndef DRNMF_SNMF_F16_H
#define DRNMF_SNMF_F16_H

#include "drnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if the kernel takes the shape: beta == 2, N even, 2 <= N <= 512, F > 0; else 0. */
int32_t drnmf_snmf_f16_admitted(int32_t F, int32_t N, float beta);

/* Bytes of the packed fp16 dictionary: F rows of N rounded up to 32 halves; 0 for F <= 0 or N <= 0. */
size_t drnmf_snmf_f16_dict_bytes(int32_t F, int32_t N);

/* Wn [F][N] fp32 -> dict16, _Float16 [F][N rounded up to 32], zero behind N (round to nearest even).  dict16: 16-byte
 * aligned, dict16_bytes >= drnmf_snmf_f16_dict_bytes (else DRNMF_ERR_WORKSPACE). */
int32_t drnmf_snmf_f16_pack_dict(drnmf_handle_t h, int32_t F, int32_t N, const float* Wn, void* dict16,
                                 size_t dict16_bytes, void* stream);

/* x [B][T][F]; dict16 as drnmf_snmf_f16_pack_dict wrote it from Wn; Wn [F][N] fp32 with unit-norm columns (8-byte
 * aligned; the numerator and the final mask read it); h_init [N] in Wn's basis; mask_out [B][T][F].  power: V =
 * x^power.  n_iter >= 0, sparsity >= 0.  N odd is DRNMF_ERR_INVALID_ARG (as in drnmf_snmf.h's entry), N > 512
 * DRNMF_ERR_UNSUPPORTED.  The entry has no beta: it computes beta == 2. */
int32_t drnmf_snmf_f16_forward(drnmf_handle_t h, int32_t B, int32_t T, int32_t F, int32_t N, int32_t n_iter,
                               float sparsity, float power, float mask_value, int32_t has_mask, const float* x,
                               const void* dict16, const float* Wn, const float* h_init, float* mask_out,
                               void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_SNMF_F16_H */
