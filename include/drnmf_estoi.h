/*
 * drnmf_estoi.h -- C ABI of the extended intelligibility score in libdrnmf.so: ESTOI beside STOI, from the same
 * band envelopes, for a ragged batch in one call.  Conventions as in drnmf_score.h: device pointers unless marked
 * host, caller-owned memory, the caller's stream, the handle's mutex, never a synchronisation, status codes,
 * drnmf_last_error.
 *
 * ESTOI [ESTOI-memory] -- Jensen & Taal, "An Algorithm for Predicting the Intelligibility of Speech Masked by
 * Modulated Noise Maskers", IEEE/ACM TASLP 24(11), 2016.  The paper's Matlab code is not part of the reference
 * repository, as the STOI toolbox is not; this is a restatement of the published algorithm, pinned in
 * tests/estoi_ref.py.  x = reference (clean), y = estimate.
 *   1-3. as drnmf_score.h: resample to 10 kHz, drop the frames of x that lie 40 dB or more below its loudest,
 *        take the band envelopes env_x, env_y [nf][15] of the compacted signals.
 *   4'.  Segment m = 0 .. nf - 30 holds band frames m .. m + 29.  Let X, Y be its 15 x 30 matrices (band by
 *        frame).  rc(A), in this order: subtract from every row (band) its mean over the 30 frames; divide every
 *        row by its Euclidean norm; subtract from every column (frame) its mean over the 15 bands; divide every
 *        column by its Euclidean norm.  d_m = sum(rc(X) * rc(Y)) / 30, ESTOI = mean_m d_m.
 * Edge semantics follow drnmf_score.h's choice for STOI: plain arithmetic, no noise term or epsilon as pystoi
 * adds.  Fewer than 30 band frames -> NaN.  A zero norm is 0 / 0 = NaN and reaches the mean: a band that is
 * constant over 30 frames, or a digitally silent stretch of the estimate, scores NaN for the whole signal (where
 * STOI, through Matlab's min, scores such a segment 1).  x against itself scores 1.
 */
#ifndef DRNMF_ESTOI_H
#define DRNMF_ESTOI_H

#include "drnmf_score.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of drnmf_stoi_ext for n_sig signals of at most max_len samples at fs (0 when fs is unsupported); at
 * least drnmf_stoi_workspace_bytes of the same arguments. */
size_t drnmf_stoi_ext_workspace_bytes(int32_t n_sig, int64_t max_len, int32_t fs);

/* STOI, ESTOI or both of n_sig pairs; the envelopes are computed once.  Arguments as drnmf_stoi.  stoi_out,
 * estoi_out [n_sig] float32, either may be NULL (not computed), both NULL is DRNMF_ERR_INVALID_ARG; stoi_out
 * receives the bits drnmf_stoi writes.  d_ext_out [n_sig][S] float64 or NULL: the per-segment d_m, S =
 * max(V - 30, 1), V = drnmf_stoi_vad_frames(max length, fs); entries past a signal's own segments are not
 * written.  workspace: 256-byte aligned, >= drnmf_stoi_ext_workspace_bytes(n_sig, max length, fs) (else
 * DRNMF_ERR_WORKSPACE); an unsupported fs is DRNMF_ERR_UNSUPPORTED.  Each row's results are independent of the
 * rest of the batch and bitwise reproducible. */
int32_t drnmf_stoi_ext(drnmf_handle_t h, int32_t n_sig, int64_t stride, const int64_t* lengths_host, int32_t fs,
                       const float* est, const float* ref, float* stoi_out, float* estoi_out, uint8_t* keep_out,
                       float* env_ref_out, float* env_est_out, double* d_ext_out, void* workspace,
                       size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_ESTOI_H */
