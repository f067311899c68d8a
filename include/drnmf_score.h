/*
 * drnmf_score.h -- C ABI of the intelligibility score in libdrnmf.so: STOI, the last column of compute_scores
 * (score_audio.m:231, `stoi(xref, xest, fs_est)`), for a ragged batch in one call.  Conventions as in drnmf.h:
 * device pointers unless marked host, caller-owned memory (nothing is allocated inside an enqueue call), the
 * caller's stream, the handle's mutex, never a synchronisation, status codes.
 *
 * STOI [STOI-memory] -- the toolbox (Taal et al., IEEE TASLP 19(7), 2011) is not part of the reference
 * repository; this is a restatement of the published algorithm, pinned in tests/stoi_ref.py.  x = reference
 * (clean), y = estimate; constants fs = 10000, frame 256, FFT 512, 15 one-third-octave bands from 150 Hz,
 * 30-frame segments, beta = -15 dB, 40 dB silence range:
 *   1. resample to 10 kHz as Matlab resample(x, 10000, fs) (N = 10, Kaiser beta = 5, delay compensated);
 *   2. drop the frames (hop 128, Matlab hanning(256), starts <= len - 257) of x whose energy is 40 dB or more
 *      below its loudest frame; overlap-add the kept windowed frames of x and of y (x's decision);
 *   3. band envelopes: 512-point FFT of every windowed frame of the compacted signals, sqrt of the band sums
 *      of |X|^2;
 *   4. for every 30-frame segment and band: Y' = min(alpha Y, X (1 + 10^(15/20))), alpha = |X| / |Y|, and
 *      d = corr(X, Y'); STOI = mean d.
 * Edge semantics are Matlab's, not pystoi's: fewer than 30 band frames (too short, or too little kept) -> NaN;
 * min ignores NaN (a segment with sum Y^2 = 0 scores d = 1); a zero-variance vector in corr -> NaN, which
 * propagates to the mean.
 */
#ifndef DRNMF_SCORE_H
#define DRNMF_SCORE_H

#include "drnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Frames of the silence detector for one signal of `len` samples at `fs` Hz: floor((L - 257) / 128) + 1 with
 * L = ceil(len * 10000 / fs) (0 when L < 257).  A signal has at most this many minus one band frames.  -1 when fs
 * is not supported: fs > 0 whose reduced ratio 10000/fs = p/q has max(p, q) <= 160 (8, 10, 16, 32, 48 kHz ...). */
int32_t drnmf_stoi_vad_frames(int64_t len, int32_t fs);

/* Workspace of drnmf_stoi for n_sig signals of at most max_len samples at fs (0 when fs is unsupported). */
size_t drnmf_stoi_workspace_bytes(int32_t n_sig, int64_t max_len, int32_t fs);

/* STOI of n_sig pairs.  est, ref [n_sig][stride] float32; lengths_host [n_sig] (0 <= lengths <= stride; samples
 * beyond a row's length are not read); stoi_out [n_sig] float32.  Optional outputs (NULL: not written), V =
 * drnmf_stoi_vad_frames(max length, fs): keep_out [n_sig][V] uint8, the silence decision (0 past a row's own
 * frames); env_ref_out, env_est_out [n_sig][max(V - 1, 1)][15] float32, the band envelopes (rows past a signal's
 * own band frames are not written).  workspace: 256-byte aligned, >= drnmf_stoi_workspace_bytes(n_sig,
 * max length, fs) (else DRNMF_ERR_WORKSPACE).  Each row's result is independent of the rest of the batch and
 * bitwise reproducible. */
int32_t drnmf_stoi(drnmf_handle_t h, int32_t n_sig, int64_t stride, const int64_t* lengths_host, int32_t fs,
                   const float* est, const float* ref, float* stoi_out, uint8_t* keep_out, float* env_ref_out,
                   float* env_est_out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_SCORE_H */
