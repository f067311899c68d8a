/*
 * drnmf_stream.h -- C ABI of the streaming front and back end in libdrnmf.so: B independent streams, each fed in
 * chunks of any length; a push turns the chunk into the STFT frames that have become complete and the masked
 * frames back into the samples that have become final.  The carry between pushes (input samples later frames
 * still read, partial overlap-add sums, counters) lives in a caller-owned device buffer.  Conventions as in
 * drnmf_enhance.h: device pointers, caller-owned memory (nothing is allocated inside a call), the caller's stream,
 * the handle's mutex, never a synchronisation, status codes, drnmf_last_error.  Per-stream counts arrive as
 * device arrays and the kernels clamp; no write goes beyond a row.
 *
 * Framing (util.py:171-226, causal): frame j reads samples [j hop - N, j hop) of its stream, zeros in front of
 * sample 0; output sample s is the sum of frames floor(s / hop) + 1 .. floor((s + N) / hop), added in ascending
 * order.  hop must divide N (so hop <= N).
 *
 * Counting rule.  A stream that has never been pushed has 0 frames and 0 samples.  After n samples:
 *   open:    frames = floor(n / hop) + 1,           samples = max(0, frames * hop - N);
 *   closed:  frames = drnmf_stft_frames(n, N, hop), samples = hop * (frames - 1) - N (crop = 0: what
 *            reconstruct_x returns) or min(n, that) (crop = 1): the signal is zero-padded exactly as offline.
 * A push yields frames(after) - frames(before) new frames and samples(after) - samples(before) new samples; an
 * open stream's output lags its input by N - hop .. N - 1 samples.
 *
 * Every frame is bitwise the one drnmf_stft_ragged computes for the whole signal, and every sample (float32)
 * bitwise the one drnmf_istft_ragged computes from the same frames and mask: the frame bodies are the same and a
 * carried partial sum is continued in ascending frame order.
 */
#ifndef DRNMF_STREAM_H
#define DRNMF_STREAM_H

#include "drnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Totals of one stream after n_samples samples (closed: 0 open, 1 closed).  Host only; no handle.  Returns
 * DRNMF_OK, or DRNMF_ERR_INVALID_ARG for n_samples < 0, N or hop < 1, hop not dividing N, closed / crop outside
 * {0, 1} or a NULL pointer. */
int32_t drnmf_stream_counts(int64_t n_samples, int32_t closed, int32_t N, int32_t hop, int32_t crop,
                            int64_t* frames, int64_t* samples);

/* Bytes of the state of B streams (0 for arguments the entry points below refuse).  Per stream: a 64-byte header
 * (int64 samples consumed, int64 frames emitted, int64 first frame and int32 frame count of the latest push,
 * int32 closed), N 32-bit words of input carry (fewer than N are in use), N - hop float32 partial overlap-add
 * sums, N float32 of frame scratch; rounded up to 64 bytes. */
size_t drnmf_stream_state_bytes(int32_t B, int32_t N, int32_t hop);

/* Zero the state: every stream fresh and open.  One launch. */
int32_t drnmf_stream_reset(drnmf_handle_t h, int32_t B, int32_t N, int32_t hop, void* state, size_t state_bytes,
                           void* stream);

/* One push, forward.  chunk [B][stride] int16 (is_int16 = 1, scaled by 1/32768) or float32 -- one type for the
 * life of a stream; chunk_len [B] int64 (taken into [0, stride]; 0 for a closed stream); final [B] int32, not 0:
 * the stream ends with this chunk (it stays closed until the reset).  Outputs, contiguous [B][T][F], F = N/2+1,
 * row b holding its stream's n_b new frames in order:
 *   x        magnitude for t < n_b, mask_value in every bin for n_b <= t < T;
 *   re, im   as drnmf_stft_ragged writes them for t < n_b; rows behind are not written.
 * New frames at or behind T are dropped (and lost: size T by the counting rule).  Then the carry and the
 * counters are updated.  N a power of two in [64, 4096], hop dividing N, 1 <= B <= 65535, T >= 1, stride >= 1. */
int32_t drnmf_stream_forward(drnmf_handle_t h, int32_t B, int64_t stride, int32_t T, int32_t N, int32_t hop,
                             int32_t is_int16, float mask_value, const void* chunk, const int64_t* chunk_len,
                             const int32_t* final, float* x, float* re, float* im, void* state,
                             size_t state_bytes, void* stream);

/* One push, inverse: exactly one call after each drnmf_stream_forward whose T it shares (it reads that push's
 * frame range from the state).  re, im [B][T][F]; mask [B][T] rows of ld_mask >= F floats (the model's output,
 * taken in place) or NULL.  The new frames are transformed and windowed as drnmf_istft_ragged does and added to
 * the carried partial sums in ascending frame order; row b of y receives the samples that have become final,
 * zeros behind them up to stride_y, and the rest stays in the state.  crop as in drnmf_istft_ragged (it matters
 * for the push that closes a stream).
 *   out_int16 = 0: y float32 [B][stride_y];
 *   out_int16 = 1: y int16 [B][stride_y] = (int16)(int)(clamp(v * 32767, -32767, 32767)), truncated toward zero:
 *     drnmf_wav_int16's arithmetic WITHOUT util.wavwrite's division by the file's peak (a stream does not know
 *     its peak before it ends).  Equal to drnmf_wav_int16_rows whenever the utterance's peak is <= 1. */
int32_t drnmf_stream_inverse(drnmf_handle_t h, int32_t B, int32_t T, int32_t N, int32_t hop, const float* re,
                             const float* im, const float* mask, int64_t ld_mask, int32_t crop,
                             int32_t out_int16, void* y, int64_t stride_y, void* state, size_t state_bytes,
                             void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_STREAM_H */
