/*
 * drnmf_target.h -- C ABI of the training targets in libdrnmf.so: drnmf_stft_pair_chunks (drnmf_dataset.h) with
 * a choice of what the clean side's tensor y holds.  Every model here predicts a mask that is applied to the noisy
 * magnitude and put back on the NOISY phase; the phase-sensitive target (Erdogan, Hershey, Watanabe, Le Roux,
 * ICASSP 2015) is the clean magnitude projected on that phase, |S| cos(theta_S - theta_X), the value such a
 * mask can reach.  Conventions as in drnmf_dataset.h: device pointers, caller-owned memory, no workspace, the
 * caller's stream, the handle's mutex, never a synchronisation, status codes, drnmf_last_error.
 *
 * For a valid frame let re_x, im_x (noisy) and re_s, im_s (clean) be what drnmf_stft / drnmf_stft_ragged write
 * for that signal and frame, and m_x = sqrtf(re_x^2 + im_x^2) the magnitude as they write it.  In float32, two
 * products, one sum and one true division, each rounded once:
 *   p = (re_s * re_x + im_s * im_x) / m_x   where m_x > 0,
 *   p = 0                                   where m_x == 0 (also where the noisy signal has ended and reads as
 *                                           zeros).
 * No spectrum goes through memory: the noisy member's bins wait on chip while the clean member is transformed.
 */
#ifndef DRNMF_TARGET_H
#define DRNMF_TARGET_H

#include "drnmf_dataset.h"

#ifdef __cplusplus
extern "C" {
#endif

/* target: what y holds in a valid frame */
#define DRNMF_TARGET_MAG 0  /* the transformed clean magnitude: drnmf_stft_pair_chunks itself, the same bits */
#define DRNMF_TARGET_PSA 1  /* p; may be negative and may exceed x */
#define DRNMF_TARGET_TPSA 2 /* min(max(p, 0), x), the part of p a mask in [0, 1] can reach */

/* drnmf_stft_pair_chunks with `target` behind `transform`.  x and w are what that call writes, bit for bit, for
 * every target; padding frames hold mask_value in x and y with weight 0.  DRNMF_TARGET_PSA and _TPSA are defined
 * for DRNMF_TRANSFORM_MAG only: with _LOGMAG, or with a target that is none of the three, the call returns
 * DRNMF_ERR_INVALID_ARG and enqueues nothing.  A p in a valid frame may equal mask_value; w tells the frames
 * apart, y never does. */
int32_t drnmf_stft_pair_chunks_target(drnmf_handle_t h, int32_t n_sig, int64_t stride_x, int64_t stride_y,
                                      const int64_t* len_x, const int64_t* len_y, int32_t n_seq,
                                      const int32_t* seq_table, int32_t T, int32_t N, int32_t hop,
                                      int32_t is_int16, int32_t transform, int32_t target, float mask_value,
                                      const void* pcm_x, const void* pcm_y, float* x, float* y, float* w,
                                      void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_TARGET_H */
