/*
 * drnmf_enhance.h -- C ABI of the ragged front and back end of the enhancement loop in libdrnmf.so
 * (enhance.py:1181-1203, audio_dataset.py:267-339): the STFT of a batch of waveforms of DIFFERENT lengths
 * straight into the model's padded [b][T][F] layout, the masked inverse STFT back into per-signal rows, and
 * util.wavwrite's int16 conversion per row.  Conventions as in drnmf.h: device pointers, caller-owned memory
 * (nothing is allocated inside a call), the caller's stream, the handle's mutex, never a synchronisation,
 * status codes, drnmf_last_error.
 *
 * The lengths live on the DEVICE (int64 [n_sig]), so a call only enqueues and the host cannot check them: the
 * kernels clamp instead.  A length is taken into [0, stride]; an entry of sig_index outside [0, n_sig) makes
 * its slab row an all-padding row (forward) or is skipped (inverse); no write goes beyond a row.
 *
 * Slabs.  The signals are pcm [n_sig][stride]; a slab is b rows chosen by the gather list sig_index [b] (int32,
 * device): slab row k belongs to signal sig_index[k].  T is the slab's frame capacity, F = N/2 + 1, and
 *   nf_k = drnmf_stft_frames(lengths[sig_index[k]], N, hop)
 * is evaluated on the device.  Frames at or behind T are dropped by both transforms.
 *
 * Every result of a signal is a fixed-order computation on that signal alone: it is bitwise the same in any
 * batch, slab position, T and run.
 */
#ifndef DRNMF_ENHANCE_H
#define DRNMF_ENHANCE_H

#include "drnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Ragged forward STFT (framing, window and arithmetic of drnmf_stft).  pcm [n_sig][stride] int16 (is_int16 = 1,
 * scaled by 1/32768) or float32; stride and the buffer's alignment may be odd.  Outputs, contiguous [b][T][F]:
 *   x    magnitude for t < nf_k; mask_value in every bin for nf_k <= t < T (the reference's padding,
 *        audio_dataset.py:144-146);
 *   re, im   the conjugated convention of drnmf_stft for t < nf_k; rows at or behind nf_k are NOT written
 *        (not zeroed) and never read by drnmf_istft_ragged.
 * N a power of two in [64, 4096], hop > 0, T >= 1, 1 <= b <= 65535, n_sig >= 1, stride >= 1. */
int32_t drnmf_stft_ragged(drnmf_handle_t h, int32_t n_sig, int64_t stride, const int64_t* lengths,
                          int32_t b, const int32_t* sig_index, int32_t T, int32_t N, int32_t hop,
                          int32_t is_int16, float mask_value, const void* pcm, float* x, float* re, float* im,
                          void* stream);

/* Ragged masked inverse: y[sig_index[k]][s] = istft_noDiv(mask_k * (re_k + i im_k))[s], the N padding samples
 * trimmed as istft_mc does, for s < nsampl_out_k, and 0 for nsampl_out_k <= s < stride_y.
 *   crop = 0: nsampl_out_k = hop * (nf_k - 1) - N = ceil(len_k / hop) * hop when hop divides N: what
 *             reconstruct_x returns (enhance.py:1199-1203 writes it to disk);
 *   crop = 1: nsampl_out_k = min(len_k, the above).
 * Either is clamped to stride_y.  re, im [b][T][F]; mask [b][T] rows of ld_mask >= F floats (the model's
 * output, taken in place) or NULL; y [n_sig][stride_y].  Only rows named by sig_index are written.
 * N = 512 and 1024 with hop <= N run one fused kernel (one wave per frame, the overlap-add in registers, every
 * sample written once) and need no workspace; other sizes go through a [b][T][N] frames buffer. */
size_t drnmf_istft_ragged_workspace_bytes(int32_t b, int32_t T, int32_t N, int32_t hop);
int32_t drnmf_istft_ragged(drnmf_handle_t h, int32_t n_sig, int32_t b, int32_t T, int32_t N, int32_t hop,
                           const int64_t* lengths, const int32_t* sig_index, const float* re, const float* im,
                           const float* mask, int64_t ld_mask, float* y, int64_t stride_y, int32_t crop,
                           void* workspace, size_t workspace_bytes, void* stream);

/* util.wavwrite's float32 -> int16 (util.py:37-45) applied to every row as to a file of its own: row k is
 * divided by max |y[k][:len_k]| if that exceeds 1, scaled by 32767 and truncated toward zero, in the float32
 * arithmetic of drnmf_wav_int16; out[k][i] = 0 for len_k <= i < stride.  y, out [n_sig][stride]; lengths
 * [n_sig] int64 on the device; workspace: one float per row (the peaks). */
size_t drnmf_wav_int16_rows_workspace_bytes(int32_t n_sig);
int32_t drnmf_wav_int16_rows(drnmf_handle_t h, int32_t n_sig, int64_t stride, const int64_t* lengths,
                             const float* y, int16_t* out, void* workspace, size_t workspace_bytes,
                             void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_ENHANCE_H */
