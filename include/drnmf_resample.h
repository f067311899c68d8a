/*
 * drnmf_resample.h -- C ABI of the device-side rational-rate resampler in libdrnmf.so: a ragged batch of
 * waveforms at fs_in converted to fs_out by one polyphase FIR pass, so that corpora and recordings at other rates
 * (noise and RIR collections at 48 or 44.1 kHz, telephone speech at 8 kHz) reach the banks and `enhance` without
 * a round trip over the host.  The reference has no such code; the definition below is this project's,
 * generalised from step 1 of drnmf_score.h (Matlab's `resample`, which STOI applies on its way to 10 kHz).
 * Conventions as in drnmf_mix.h and drnmf_reverb.h: device pointers, caller-owned memory, the caller's stream, the
 * handle's mutex, never a synchronisation, status codes, drnmf_last_error; lengths that live on the device are
 * clamped into [0, stride] by the kernel.
 *
 * Rate.  p / q = fs_out / fs_in, reduced by their gcd.  fs <= 0 and max(p, q) > DRNMF_RESAMPLE_MAX_PQ are refused
 * (DRNMF_ERR_INVALID_ARG; the size queries return 0).  640 admits 11025 <-> 16000 (640 / 441), 44100 <-> 16000
 * (160 / 441) and 44100 <-> 48000 (147 / 160).
 *
 * Filter.  M = max(p, q), L = 2 nz M + 1, half = (L - 1) / 2; nz >= 1 (default DRNMF_RESAMPLE_NZ = 10), beta >= 0
 * and finite (default DRNMF_RESAMPLE_BETA = 5.0):
 *   h[i] = kaiser_beta(i) sinc((i - half) / M) / M,   kaiser_beta(i) = I0(beta sqrt(1 - ((i - half) / half)^2)) / I0(beta)
 * then scaled so that sum h = p.  drnmf_resample_taps computes it on the device in fp64 (one workgroup, a fixed
 * summation tree: the bits depend on (p, q, nz, beta) alone); the caller keeps the table, L doubles, for as long
 * as it likes.  nz is limited by the LDS of a compute unit, which must hold the table and the samples one output
 * meets: drnmf_resample_tile returns 0 where it does not (nz = 10 fits at every admitted rate).
 *
 * Output.  A signal x of n samples gives ceil(n p / q) outputs
 *   y[m] = sum_k x[k] h[q m + half - p k]      over the k in [0, n) whose tap index lies in [0, L)
 * as ONE chain acc = fma((double)x[k], h[.], acc) in fp64, ascending in k from +0.0, rounded once to float32.
 * An int16 sample is (float)v / 32768.0f.  p == q == 1 is a copy, bit for bit (int16 converted as above), and
 * reads no filter (taps may be NULL).
 *
 * Layout.  in [n_sig][stride_in], int16 (is_int16 = 1) or float32; len int64 [n_sig] on the DEVICE; out float32
 * [n_sig][stride_out].  Every element of out is written: 0.0f from the signal's output length on (outputs beyond
 * stride_out are dropped).  Strides and base alignments may be odd.  No atomics.  No workgroup waits for another.
 * A signal's bits do not depend on n_sig, the strides, the alignment path taken, or the signals beside it.
 *
 * Chunked form.  drnmf_resample_chunk runs the same kernel body on a window of every signal: row i holds the
 * samples x[in_start[i] .. in_start[i] + len[i]) and the call writes the out_count[i] outputs y[out_start[i] ..]
 * to out[i][0 ..], zeros behind them.  total[i] is the signal's whole length n, which cuts the sums at k < n and
 * the outputs at m < ceil(n p / q), or -1 while it is not yet known (the samples held are then all there is).  An
 * output is final, the same bits as the offline call's, once sample floor((q m + half) / p) has arrived, and needs
 * the samples from max(0, ceil((q m + half - (L - 1)) / p)) on: the caller asks only for final outputs and keeps
 * that history in the row (terms whose sample the row does not hold are skipped).  All four tables are int64
 * [n_sig] on the DEVICE and may be NULL: in_start 0, out_start 0, out_count all of ceil(n p / q), total = len --
 * which is the offline call.
 *
 * Shape of the kernel.  One workgroup of 256 threads per (signal, tile of drnmf_resample_tile outputs): the whole
 * table (fp64) and the tile's input span (float32, int16 converted while staged) are staged once in LDS, then
 * thread t sums outputs t, t + 256, ... of the tile.  A tile is DRNMF_RESAMPLE_TILE outputs unless its input span
 * would not fit beside the table (steep decimation), then as many as do.  A tile behind the signal's last output
 * stages nothing and writes zeros.
 */
#ifndef DRNMF_RESAMPLE_H
#define DRNMF_RESAMPLE_H

#include "drnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DRNMF_RESAMPLE_MAX_PQ 640
#define DRNMF_RESAMPLE_NZ 10
#define DRNMF_RESAMPLE_BETA 5.0
#define DRNMF_RESAMPLE_TILE 2048 /* outputs per workgroup, at most */

/* p / q = fs_out / fs_in reduced.  DRNMF_ERR_INVALID_ARG (p and q left alone) for a rate <= 0 or max(p, q) >
 * DRNMF_RESAMPLE_MAX_PQ.  No handle, no device. */
int32_t drnmf_resample_rate(int64_t fs_in, int64_t fs_out, int32_t* p, int32_t* q);

/* Size queries; 0 for a refused shape (p or q outside [1, DRNMF_RESAMPLE_MAX_PQ], nz < 1, n < 0, a table that
 * leaves no room in LDS).  taps_len: L, and 0 for p == q == 1 as well (the copy has no filter).  out_len: ceil(n p /
 * q), n <= 2^40.  tile: the outputs per workgroup of the kernel (DRNMF_RESAMPLE_TILE for p == q == 1). */
int64_t drnmf_resample_taps_len(int32_t p, int32_t q, int32_t nz);
int64_t drnmf_resample_out_len(int64_t n, int32_t p, int32_t q);
int32_t drnmf_resample_tile(int32_t p, int32_t q, int32_t nz);

/* taps: drnmf_resample_taps_len(p, q, nz) doubles on the device, the filter above (p and q reduced). */
int32_t drnmf_resample_taps(drnmf_handle_t h, int32_t p, int32_t q, int32_t nz, double beta, double* taps,
                            void* stream);

/* The offline call: out [n_sig][stride_out] of the definition above; it must not overlap in.  One launch per
 * slice of 65 535 signals.  n_sig >= 1 (no upper limit), 1 <= stride_in, stride_out <= 2^40, is_int16 0 or 1, p and
 * q reduced, taps from drnmf_resample_taps with the same (p, q, nz); no workspace. */
int32_t drnmf_resample_forward(drnmf_handle_t h, int32_t n_sig, int64_t stride_in, const int64_t* len,
                               int32_t is_int16, const void* in, int32_t p, int32_t q, int32_t nz,
                               const double* taps, int64_t stride_out, float* out, void* stream);

/* The chunked form (see above); every table may be NULL, and with all four NULL this is drnmf_resample_forward. */
int32_t drnmf_resample_chunk(drnmf_handle_t h, int32_t n_sig, int64_t stride_in, const int64_t* len,
                             const int64_t* in_start, const int64_t* out_start, const int64_t* out_count,
                             const int64_t* total, int32_t is_int16, const void* in, int32_t p, int32_t q,
                             int32_t nz, const double* taps, int64_t stride_out, float* out, void* stream);

/* The history of a chunked caller, moved on between two pushes: next[i][j] = prev[i][drop[i] + j] for j < keep[i],
 * then chunk[i][j - keep[i]] for j < keep[i] + add[i]; the rest of next is left as it is.  prev [n_sig][stride_prev],
 * chunk [n_sig][stride_chunk] and next [n_sig][stride_next] hold one type (is_int16) and must not overlap; drop,
 * keep and add are int64 [n_sig] on the DEVICE, and a row's counts are clamped so that nothing outside a row is
 * read or written.  chunk may be NULL when stride_chunk is 0 (nothing is added). */
int32_t drnmf_resample_carry(drnmf_handle_t h, int32_t n_sig, int32_t is_int16, int64_t stride_prev,
                             const void* prev, int64_t stride_chunk, const void* chunk, const int64_t* drop,
                             const int64_t* keep, const int64_t* add, int64_t stride_next, void* next, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_RESAMPLE_H */
