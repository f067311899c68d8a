/*
 * drnmf_stoi_loss.h -- C ABI of the intelligibility criterion in libdrnmf.so: minus STOI of a ragged batch and
 * its exact gradient with respect to the estimate's samples, in one call.  Conventions as in drnmf_score.h:
 * device pointers unless marked host, caller-owned memory, the caller's stream, the handle's mutex, never a
 * synchronisation, status codes, drnmf_last_error.
 *
 * Training on (minus) STOI follows Fu et al., "End-to-end waveform utterance enhancement for direct evaluation
 * metrics optimization by fully convolutional neural networks", IEEE/ACM TASLP 26(9), 2018.  The gradient here is
 * that of the score drnmf_stoi computes (drnmf_score.h, steps 1-4), not of a surrogate: the silence decision and
 * the compaction index depend on the REFERENCE only, so as a function of the estimate y the score is differentiable
 * everywhere except on the clip ties and at zero envelopes.  x = reference, c = 1 + 10^(15/20), J = 15 bands,
 * S = the row's segments.  Backwards through the stages (restated in fp64 in tests/stoi_loss_ref.py):
 *   segments    For segment m and band j over its 30 frames: Sx = sum X^2, Sy = sum Y^2, alpha = sqrt(Sx / Sy),
 *               u_t = [alpha Y_t <= c X_t], Y' = u ? alpha Y : c X, x^ and y^ the centred, normalised X and Y',
 *               d = <x^, y^>.  Then g = (x^ - d y^) / ||Y' - mean|| and
 *                   dd/dY_t = alpha u_t g_t - (alpha / Sy) Y_t sum_s u_s g_s Y_s.
 *               A frame's envelope receives this from up to 30 segments; the total is scaled by -1 / (S J).
 *               A segment-band with Sy == 0 (which the forward scores 1) contributes zero gradient.
 *   envelopes   Y = sqrt(sum_{k in band} |Z_k|^2): G_k = gY Z_k / Y on the band's bins, 0 on the others and where
 *               Y == 0; the frame's sample gradient is w[n] Re sum_k G_k e^{+2 pi i k n / 512}, n < 256.
 *   compaction  Band frame i covers compacted samples 128 i .. 128 i + 255 (overlap-add into g_ys); kept frame c at
 *               source start s_c gives g_y10k[s_c + n] += w[n] g_ys[128 c + n].
 *   resampling  g_est[k] = sum_m g_y10k[m] h[q m + (L-1)/2 - p k]; skipped at 10 kHz.
 * A row is COUNTED iff its STOI is finite: a row with fewer than 30 band frames, or whose score is NaN through a
 * zero-variance band, has loss 0, gradient 0 and counted 0, so one unusable recording cannot poison a step.
 * The backward runs in fp64 as the forward does and stores float32; every sum is a gather in a fixed order (no
 * atomics), so a row's loss and gradient are bitwise the same in any batch and in every run.
 */
#ifndef DRNMF_STOI_LOSS_H
#define DRNMF_STOI_LOSS_H

#include "drnmf_score.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DRNMF_STOI_LOSS_STOI 0          /* the only kind (room for ESTOI) */

/* Workspace of drnmf_stoi_loss for n_sig signals of at most max_len samples at fs: a multiple of 256, at least
 * drnmf_stoi_workspace_bytes of the same arguments; 0 for n_sig <= 0, max_len outside [0, 2^30] or an unsupported
 * fs. */
size_t drnmf_stoi_loss_workspace_bytes(int32_t n_sig, int64_t max_len, int32_t fs);

/* est, ref [n_sig][stride] float32; lengths_host [n_sig] int64 on the HOST, each in [0, min(stride, 2^30)] (they
 * reach the device as kernel arguments: nothing is copied from pageable memory); fs as drnmf_stoi.  kind:
 * DRNMF_STOI_LOSS_STOI, anything else DRNMF_ERR_UNSUPPORTED.  Outputs: loss [n_sig] = -STOI with the bits
 * drnmf_stoi gives, negated (0 for a row that is not counted); counted [n_sig] (1.0f / 0.0f); g [n_sig][stride] =
 * d (sum of counted losses) / d est, every element written, 0 at and behind a row's length; sums [2] = {sum of
 * counted losses, their number} ({0, 0} when nothing is counted).  workspace: 256-byte aligned, >=
 * drnmf_stoi_loss_workspace_bytes(n_sig, max length, fs).  Order of the checks: arguments (n_sig in [1, 65535],
 * 0 < stride <= 2^38, lengths, NULL: DRNMF_ERR_INVALID_ARG), fs, kind (DRNMF_ERR_UNSUPPORTED), workspace
 * (DRNMF_ERR_WORKSPACE, NULL included), the device. */
int32_t drnmf_stoi_loss(drnmf_handle_t h, int32_t n_sig, int64_t stride, const int64_t* lengths_host, int32_t fs,
                        const float* est, const float* ref, int32_t kind, float* loss, float* counted, float* g,
                        float* sums, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_STOI_LOSS_H */
