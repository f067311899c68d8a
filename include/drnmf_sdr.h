/*
 * drnmf_sdr.h -- C ABI of the device-side SDR in libdrnmf.so: the first column of compute_scores
 * (score_audio.m:206, `bss_eval_sources(xest', xref')` with one source) for a ragged batch, enqueued from the
 * samples to the dB with no host step, and the batched Toeplitz solve it is built on.  Conventions as in
 * drnmf_score.h: device pointers, caller-owned memory (nothing is allocated inside a call), the caller's stream,
 * the handle's mutex, never a synchronisation, status codes, drnmf_last_error; a bad argument is refused before
 * anything is enqueued (also on a drnmf_create_unbound handle).
 *
 * The definition is the one of drnmf_sdr_corr / drnmf_sdr_project (drnmf.h): the estimate, zero-padded by
 * flen - 1 samples, is projected onto the span of the reference delayed by 0 .. flen-1 samples,
 *     r[a] = sum_n ref[n] ref[n-a],  d[a] = sum_n est[n] ref[n-a],  Toeplitz(r) c = d,
 *     s[n] = sum_a c[a] ref[n-a],    SDR = 10 log10(sum s^2 / sum (est - s)^2),
 * in fp64.  Every result of a row is a fixed-order computation on that row's own samples: bitwise the same in
 * any batch, stride, position and run.
 */
#ifndef DRNMF_SDR_H
#define DRNMF_SDR_H

#include "drnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Solve n_sys symmetric Toeplitz systems Toeplitz(r_k) c_k = d_k by the Levinson-Durbin recursion (O(n^2), one
 * wavefront per system, every dot product summed in a fixed order).  r, d, c_out [n_sys][n] float64 (r_k[a] is the
 * entry at distance a from the diagonal); info_out [n_sys] int32; 1 <= n <= 2048, n_sys >= 1.
 *   info = 0      solved;
 *   info = 1      r[0] <= 0 or not finite (a silent reference): c = 0;
 *   info = 2 + k  the prediction error stopped being positive at step k (1 <= k < n; the matrix is not positive
 *                 definite to working precision): c is the order-k solution, c[k..] = 0. */
int32_t drnmf_toeplitz_solve(drnmf_handle_t h, int32_t n_sys, int32_t n, const double* r, const double* d,
                             double* c_out, int32_t* info_out, void* stream);

/* Workspace of drnmf_sdr_ragged (0 for an empty shape or flen > 2048). */
size_t drnmf_sdr_ragged_workspace_bytes(int32_t n_sig, int64_t stride, int32_t flen);

/* SDR of n_sig pairs.  est, ref [n_sig][stride] float32; lengths [n_sig] int64 ON THE DEVICE, or NULL: every row
 * has the full stride.  A length is taken into [0, stride]; samples behind a row's length are never read, and
 * workgroups behind a row's end exit without touching memory.  sdr_out [n_sig] float32 (dB).  Optional outputs
 * (NULL: not written): coef_out, r_out, d_out [n_sig][flen] float64; energies_out [n_sig][2] float64 (sum s^2,
 * sum (est - s)^2); info_out [n_sig] int32, as drnmf_toeplitz_solve.  A silent reference (or a row of length 0)
 * has info = 1, c = 0 and SDR = -inf (NaN when the estimate is silent too).  1 <= n_sig <= 65535, stride >= 1,
 * 1 <= flen <= 2048; workspace: 256-byte aligned, >= drnmf_sdr_ragged_workspace_bytes(n_sig, stride, flen) (else
 * DRNMF_ERR_WORKSPACE). */
int32_t drnmf_sdr_ragged(drnmf_handle_t h, int32_t n_sig, int64_t stride, const int64_t* lengths_dev, int32_t flen,
                         const float* est, const float* ref, float* sdr_out, double* coef_out,
                         double* energies_out, double* r_out, double* d_out, int32_t* info_out, void* workspace,
                         size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_SDR_H */
