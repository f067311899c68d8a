/*
 * drnmf_reverb.h -- C ABI of the device-side reverberator in libdrnmf.so: every signal of a speech bank
 * convolved with one of a bank of room impulse responses (RIRs), so that multi-condition training can put its
 * speech in a room without leaving the device (the reference trains on CHiME2, whose speech was convolved with
 * measured RIRs before the noise was added).  The reference has no such code; the definition below is this
 * project's.  Conventions as in drnmf_mix.h: device pointers, caller-owned memory, the caller's stream, the
 * handle's mutex, never a synchronisation, status codes, drnmf_last_error; lengths that live on the device are
 * clamped into [0, stride] by the kernel.
 *
 * Signals.  speech [n_sig][stride_s], int16 (is_int16 = 1) or float32; rirs float32 [n_rir][stride_r]; strides
 * and alignments may be odd.  len_s int64 [n_sig], len_r int64 [n_rir], rir_index int32 [n_sig], delay int32
 * [n_rir] (NULL: 0 for every RIR) and n_early int32 [n_rir] (NULL: all taps of every RIR) live on the DEVICE.
 *
 * Definition.  Signal i has n = len_s[i] samples s[m].  An int16 sample is (float)v / 32768.0f, and s[m] = 0
 * outside [0, n).  Let:
 *   j = rir_index[i] and L = len_r[j];
 *   d = delay[j], clamped to [0, L-1];
 *   E = n_early[j], clamped to [0, L].
 * Then:
 *   e[k] = sum_{t = 0 .. E-1}  h[t] * s[k + d - t]
 *   l[k] = sum_{t = E .. L-1}  h[t] * s[k + d - t]
 *   wet[i][k]   = e[k] + l[k]   (one float32 add; exactly e[k] when E == L)      k < n
 *   early[i][k] = e[k]                                                           k < n
 *   both 0.0f for n <= k < stride_s
 * Each sum is a single chain acc = fmaf(h[t], s[.], acc), starting from +0.0f, in ascending t.  Terms whose
 * sample lies outside the signal are skipped.  If j is outside [0, n_rir) or L == 0, both outputs are the speech
 * as float32, bit for bit, and no RIR is read.  Every element of both outputs is written and none outside them.
 * No atomics.  No workgroup waits for another.  A signal's bits do not depend on n_sig, the strides, the
 * alignment path taken, or the signals beside it.
 *
 * The delay moves the output forward: with d the index of an RIR's direct-path tap, wet stays aligned with the
 * dry speech (the taps before d read ahead, up to d samples); with d = 0 the output is the causal convolution cut
 * to the signal's length.  The early part, the taps before E, is the target of a model that is to remove late
 * reverberation only.
 *
 * Shape of the kernel.  One workgroup of 256 threads per (signal, tile of DRNMF_REVERB_TILE outputs); it walks
 * the taps in chunks of DRNMF_REVERB_CHUNK, counted from tap 0, and skips the chunks that cannot touch the signal.
 */
#ifndef DRNMF_REVERB_H
#define DRNMF_REVERB_H

#include "drnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DRNMF_REVERB_TILE 2048  /* outputs per workgroup */
#define DRNMF_REVERB_CHUNK 1024 /* taps staged at a time */

/* wet (and early, unless NULL) of the definition above, float32 [n_sig][stride_s] each; they must not overlap
 * speech or each other.  One launch per slice of 65 535 signals.  n_sig >= 1 and n_rir >= 1 (n_sig has no upper
 * limit), stride_s >= 1, 1 <= stride_r <= 2^30, is_int16 0 or 1; no workspace. */
int32_t drnmf_reverb_forward(drnmf_handle_t h, int32_t n_sig, int64_t stride_s, const int64_t* len_s,
                             int32_t is_int16, const void* speech, int32_t n_rir, int64_t stride_r,
                             const int64_t* len_r, const float* rirs, const int32_t* rir_index, const int32_t* delay,
                             const int32_t* n_early, float* wet, float* early, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_REVERB_H */
