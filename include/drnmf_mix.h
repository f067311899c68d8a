/*
 * drnmf_mix.h -- C ABI of the device-side mixer in libdrnmf.so: noisy = speech + g * noise at a requested
 * signal-to-noise ratio, for multi-condition training from a speech bank and a noise bank that stay on the
 * device.  The reference has no mixing code (it trains on CHiME2's ready-made mixtures); the definition below is
 * this project's.  Conventions as in drnmf_dataset.h: device pointers, caller-owned memory, the caller's stream,
 * the handle's mutex, never a synchronisation, status codes, drnmf_last_error; lengths that live on the device
 * are clamped into [0, stride] by the kernels.
 *
 * Signals.  speech [n_sig][stride_s] and noise [n_noise][stride_n], each int16 (is_int16 = 1; a sample is
 * (float)v / 32768.0f) or float32, the two sides independently; strides and alignments may be odd.  len_s
 * int64 [n_sig] and len_n int64 [n_noise] live on the DEVICE.
 *
 * Definition.  Signal i has n = len_s[i] samples s[k]; its noise is j = noise_index[i] with L = len_n[j] samples,
 * read from o = offset[i] mod L (taken into [0, L), so a negative offset counts from the end) and wrapped as
 * often as needed:
 *   seg[k] = noise[j][(o + k) mod L]                           k < n
 *   Es = sum_k s[k]^2,  En = sum_k seg[k]^2                    fp64 sums of the float32 sample values
 *   g  = sqrt(Es / En) * 10^(-snr_db[i] / 20)                  in fp64, rounded once to float32
 *   noisy[i][k] = fmaf(g, seg[k], s[k])  for k < n,  0.0f  for n <= k < stride_s.
 * g = 0, and the mixture is the speech itself bit for bit, whenever Es == 0, En == 0, L == 0, j is outside
 * [0, n_noise), snr_db[i] is not finite or g is not finite.  Energies run over the whole signal: there is no
 * speech-activity weighting.  Every element of noisy is written, none outside it.
 *
 * Order of the sums.  A signal is cut into blocks of 4096 samples counted from its own sample 0.  Thread t of
 * the 256 of a block adds the squares of samples 1024 c + 4 t + e (c = 0..3 outer, e = 0..3 inner) in that
 * order; the 64 partial sums of a wave go through a fixed butterfly (lane distances 32, 16, 8, 4, 2, 1), the four
 * waves are added in wave order, and the blocks' partial sums in ascending block order.  No atomics, no
 * workgroup waits for another: a signal's Es, En, g and samples have the same bits whatever n_sig, the strides,
 * its position in the batch and the signals beside it.
 */
#ifndef DRNMF_MIX_H
#define DRNMF_MIX_H

#include "drnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DRNMF_MIX_BLOCK 4096 /* samples per partial sum */

/* Bytes of workspace drnmf_mix_energy and drnmf_mix_forward need for n_sig signals of stride_s samples: the
 * per-block fp64 partial sums of both energies, and per signal the speech energy (when the call computes it)
 * and the gain.  A multiple of 256; 0 for a shape the calls refuse. */
size_t drnmf_mix_workspace_bytes(int32_t n_sig, int64_t stride_s);

/* energy[i] = sum_{k < len[i]} pcm[i][k]^2 (fp64 [n_sig] on the device), in the order above: what
 * drnmf_mix_forward takes as speech_energy.  n_sig >= 1 (no upper limit: the call splits its launches),
 * stride >= 1, is_int16 0 or 1; workspace of drnmf_mix_workspace_bytes(n_sig, stride). */
int32_t drnmf_mix_energy(drnmf_handle_t h, int32_t n_sig, int64_t stride, const int64_t* len, int32_t is_int16,
                         const void* pcm, double* energy, void* workspace, size_t workspace_bytes, void* stream);

/* The mixtures of the definition above.  noise_index int32 [n_sig], offset int64 [n_sig], snr_db float32
 * [n_sig] on the device.  speech_energy: drnmf_mix_energy of the speech side, or NULL (computed here, to the
 * same bits).  noisy float32 [n_sig][stride_s]; gain float32 [n_sig] or NULL.  Launches: the segment-energy
 * partial sums per (signal, block), one launch that adds them and writes g, the mix.  n_sig >= 1 and
 * n_noise >= 1 (no upper limit), stride_s >= 1, stride_n >= 1, the two is_int16 flags 0 or 1; workspace of
 * drnmf_mix_workspace_bytes(n_sig, stride_s). */
int32_t drnmf_mix_forward(drnmf_handle_t h, int32_t n_sig, int64_t stride_s, const int64_t* len_s,
                          int32_t s_is_int16, const void* speech, int32_t n_noise, int64_t stride_n,
                          const int64_t* len_n, int32_t n_is_int16, const void* noise, const int32_t* noise_index,
                          const int64_t* offset, const float* snr_db, const double* speech_energy, float* noisy,
                          float* gain, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_MIX_H */
