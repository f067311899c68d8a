/*
 * drnmf_waveloss.h -- C ABI of the waveform criteria in libdrnmf.so: a loss on the masked inverse STFT's
 * samples (MSE or SI-SDR), the transpose of that inverse (waveform cotangent -> mask cotangent) and the two
 * mask heads' backward passes for a GIVEN mask cotangent.  Conventions as in drnmf.h: device pointers,
 * caller-owned memory (nothing is allocated inside a call), the caller's stream, the handle's mutex, never a
 * synchronisation, status codes, drnmf_last_error.  Ragged batches as in drnmf_enhance.h: lengths [n_sig]
 * int64 and sig_index [b] int32 live on the device and are clamped there.
 *
 * The identity behind drnmf_istft_ragged_vjp.  With s^ = istft_noDiv(m * (re + i im)) (drnmf_istft_ragged,
 * any crop) and g a cotangent of s^ (0 at and behind the row's output length), let G = STFT(g) on the forward
 * frame grid (output sample s at padded position s + N, frames 0 .. n_frames-1, the same window).  Then
 *     d_mask[t][f] = (c_f / N) (2 hop / N) (re[t][f] Re G[t][f] + im[t][f] Im G[t][f]),
 *     c_0 = c_{N/2} = 1, c_f = 2 otherwise,
 * in the conjugated convention drnmf_stft stores: the inverse's transpose is the forward frame body with
 * another epilogue.
 *
 * Sums.  Every gradient is that of the SUM of the counted rows' losses (the unnormalised convention of
 * drnmf_loss_head_backward); sums[2] = {sum of counted losses, number of counted rows} is what a trainer
 * divides by.
 */
#ifndef DRNMF_WAVELOSS_H
#define DRNMF_WAVELOSS_H

#include "drnmf.h"
#include "drnmf_lstm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DRNMF_WAVE_LOSS_MSE 0
#define DRNMF_WAVE_LOSS_SI_SDR 1
#define DRNMF_WAVE_LOSS_BLOCK 4096      /* samples per partial sum of drnmf_wave_loss */

/* Transpose of drnmf_istft_ragged with respect to its mask.  g [n_sig][ld_g] float32: row sig_index[k] is the
 * cotangent of slab row k's reconstruction; samples at or behind the row's output length (as
 * drnmf_istft_ragged defines it for this crop, clamped to ld_g) count as 0 and are never read.  re, im
 * [b][T][F] as drnmf_stft_ragged wrote them, F = N/2 + 1.  d_mask [b][T] rows of ld_dm >= F floats: the formula
 * above for t < min(nf_k, T), 0 for the frames behind it, for a row whose sig_index lies outside [0, n_sig)
 * and in the columns F .. ld_dm-1.  One kernel: the windowed frame of g, its transform and the product with
 * the stored spectrum; no workspace.  N a power of two in [64, 4096], hop > 0, T >= 1, 1 <= b <= 65535,
 * crop 0 or 1, ld_g >= 1.  A row's d_mask is a fixed-order computation on that row alone: bitwise the same in
 * any batch.  Order of the checks: shape, N, NULL, ld_dm (all DRNMF_ERR_INVALID_ARG, as drnmf_istft_ragged). */
int32_t drnmf_istft_ragged_vjp(drnmf_handle_t h, int32_t n_sig, int32_t b, int32_t T, int32_t N, int32_t hop,
                               const int64_t* lengths, const int32_t* sig_index, const float* re,
                               const float* im, const float* g, int64_t ld_g, int32_t crop, float* d_mask,
                               int64_t ld_dm, void* stream);

/* Per-row waveform loss and its gradient.  est, ref, g [n_sig][ld] float32; lengths [n_sig] int64 on the
 * device, each taken into [0, ld]: n = a row's valid samples.  With p = <est, ref>, q = |ref|^2, e = |est|^2
 * over those n samples (fp64, a fixed order: 16 consecutive terms per lane, DRNMF_WAVE_LOSS_BLOCK per
 * workgroup, the blocks in ascending order):
 *   kind = DRNMF_WAVE_LOSS_MSE      loss = (1/n) sum (est - ref)^2; counted when n >= 1;
 *   kind = DRNMF_WAVE_LOSS_SI_SDR   loss = -10 log10((p^2/q + eps) / (e - p^2/q + eps)), eps = 1e-8; counted
 *                                   when n >= 1 and q > 0 (a digitally silent reference is not).
 * A row that is not counted has loss 0 and g = 0.  Outputs: loss [n_sig], counted [n_sig] (1.0f / 0.0f),
 * g = d (sum of counted losses) / d est, 0 at and behind n, and sums [2] = {sum of counted losses, their
 * number}.  Order of the checks: shape, kind, NULL (INVALID_ARG), workspace (DRNMF_ERR_WORKSPACE). */
size_t drnmf_wave_loss_workspace_bytes(int32_t n_sig, int64_t ld);
int32_t drnmf_wave_loss(drnmf_handle_t h, int32_t n_sig, int64_t ld, const int64_t* lengths, const float* est,
                        const float* ref, int32_t kind, float* loss, float* counted, float* g, float* sums,
                        void* workspace, size_t workspace_bytes, void* stream);

/* drnmf_loss_head_backward for a given cotangent of the mask: d_mask [rows] rows of ld_dm >= F floats takes
 * the place of x_raw, mask, y, w (no loss is evaluated, no sums are written).  mask = (eps + A) / (eps + A +
 * Bn), A and Bn [rows][F] as drnmf_head_forward returned them; d_hidden [rows][2r], d_kernel_clean,
 * d_kernel_noise [r][F].  workspace: drnmf_loss_head_workspace_bytes(rows, F, r).  Checks in the order of
 * drnmf_loss_head_backward: shape (ld_dm included), NULL, workspace. */
int32_t drnmf_head_backward_cot(drnmf_handle_t h, int64_t rows, int32_t F, int32_t r, const float* hidden,
                                int64_t ld_h, int32_t h_off, const float* kernel_clean,
                                const float* kernel_noise, int32_t square, const float* A, const float* Bn,
                                const float* d_mask, int64_t ld_dm, float* d_hidden, float* d_kernel_clean,
                                float* d_kernel_noise, void* workspace, size_t workspace_bytes, void* stream);

/* drnmf_lstm_loss_head_backward for a given cotangent of the sigmoid head's output s [B][T][F]: dpre = d_mask
 * s (1 - s), then the same three products (d_hidden [B][T][H], d_w_out [H][F], d_b_out [F]).  After
 * drnmf_lstm_train_forward on the same workspace, before drnmf_lstm_backward.  d_mask [B T] rows of ld_dm >= F
 * floats.  Refuses operand_f16 = 1 (DRNMF_ERR_UNSUPPORTED) as every training entry does; the other checks in
 * the order of drnmf_lstm_loss_head_backward, ld_dm last. */
int32_t drnmf_lstm_head_backward_cot(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* d_mask,
                                     int64_t ld_dm, const float* hidden, int32_t ld_h, const void* params,
                                     const float* w_out, float* d_hidden, float* d_w_out, float* d_b_out,
                                     void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_WAVELOSS_H */
