/*
 * drnmf_dataset.h -- C ABI of the training-data front end in libdrnmf.so: the reference's route from waveform
 * pairs to the tensors it trains on (audio_dataset.py:20-88 load_from_wavfiles, 116-169 get_padded_data_matrix,
 * 199-264 load_data) as one enqueue.  For every (noisy, clean) pair: the STFT magnitude of both, the noisy side
 * clipped to the clean side's frame count, the 'mag' / 'logmag' transform, the cut into consecutive sequences
 * of at most T frames padded with the mask value, and the 0/1 weights -- or, for the SNMF branch, the unpadded
 * frames of both sides as packed rows.  Conventions as in drnmf_enhance.h: device pointers, caller-owned
 * memory (nothing is allocated inside a call and neither call needs a workspace), the caller's stream, the
 * handle's mutex, never a synchronisation, status codes, drnmf_last_error.
 *
 * Signals.  pcm_x [n_sig][stride_x] (noisy) and pcm_y [n_sig][stride_y] (clean), int16 (is_int16 = 1, scaled by
 * 1/32768) or float32, both of the same type; strides and alignments may be odd.  len_x, len_y int64 [n_sig]
 * live on the DEVICE, so the host cannot check them: the kernels clamp.  A length is taken into [0, stride].
 *
 * Frames.  F = N/2 + 1 and, evaluated on the device,
 *   nf_s = drnmf_stft_frames(len_y[s], N, hop):
 * the CLEAN side decides how many frames a pair has (fidx = y_fidx in the reference).  The noisy signal is
 * framed with its OWN length: one that is longer than its clean partner contributes its real samples to the
 * last frames, exactly as clipping its full STFT does; behind its own length it reads as zeros.
 *
 * A magnitude is bitwise what drnmf_stft / drnmf_stft_ragged write for that signal and frame.  A result depends
 * on its own signal only: it is bitwise the same at any table position, for any T and on any run.  No re / im is
 * produced.
 */
#ifndef DRNMF_DATASET_H
#define DRNMF_DATASET_H

#include "drnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* transform: */
#define DRNMF_TRANSFORM_MAG 0    /* m = sqrt(re^2 + im^2)                       (audio_dataset.py:22-23) */
#define DRNMF_TRANSFORM_LOGMAG 1 /* logf(1.0f + m), the reference's expression  (audio_dataset.py:24-25) */

/* Padded sequences, the layout fit() takes.  seq_table [n_seq][2] int32 on the device: row k = (signal s_k,
 * first frame f_k).  Outputs, contiguous, for t in [0, T):
 *   x, y [n_seq][T][F]   the transformed magnitude of frame f_k + t of the noisy / the clean signal where
 *                        f_k + t < nf_s, mask_value in every bin elsewhere;
 *   w    [n_seq][T]      1.0f in the first case, 0.0f in the second (fit's sample_weight).
 * A table row whose signal is outside [0, n_sig) or whose first frame is negative gives an all-padding
 * sequence with zero weights.  Every element of x, y and w is written, none outside them.
 * N a power of two in [64, 4096], hop > 0, T >= 1, n_seq >= 1 (no upper limit: the call splits its launches),
 * n_sig >= 1, stride_x >= 1, stride_y >= 1, is_int16 0 or 1. */
int32_t drnmf_stft_pair_chunks(drnmf_handle_t h, int32_t n_sig, int64_t stride_x, int64_t stride_y,
                               const int64_t* len_x, const int64_t* len_y, int32_t n_seq,
                               const int32_t* seq_table, int32_t T, int32_t N, int32_t hop, int32_t is_int16,
                               int32_t transform, float mask_value, const void* pcm_x, const void* pcm_y,
                               float* x, float* y, float* w, void* stream);

/* Packed frames, the row layout drnmf_mu_forward and the dictionary trainer take (masked_seqs_to_frames of the
 * padded tensors, transposed).  row0 int64 [n_sig] on the device: the caller's exclusive prefix sum of the
 * frame counts nf_s.  Frame t < nf_s of signal s goes to row row0[s] + t of x_frames / y_frames
 * [total_frames][F]; nothing else is written, and a row outside [0, total_frames) is dropped. */
int32_t drnmf_stft_pair_frames(drnmf_handle_t h, int32_t n_sig, int64_t stride_x, int64_t stride_y,
                               const int64_t* len_x, const int64_t* len_y, const int64_t* row0,
                               int64_t total_frames, int32_t N, int32_t hop, int32_t is_int16,
                               int32_t transform, const void* pcm_x, const void* pcm_y, float* x_frames,
                               float* y_frames, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_DATASET_H */
