// The Kaiser-windowed sinc of Matlab's `resample`, on the device in fp64: the taps of step 1 of
// include/drnmf_score.h (STOI's resampling to 10 kHz, stoi.hip) and of include/drnmf_resample.h (resample.hip).
//   h[i] = kaiser_beta(i) sinc((i - half) / mpq) / mpq,  i in [0, L), half = (L - 1) / 2, mpq = max(p, q),
// then scaled so that sum h = p.  One workgroup of 256 threads computes a filter; the sum is a fixed tree over
// the threads' strided partial sums, so a filter's bits depend on (p, mpq, L, beta) alone.
#pragma once
#include "common.h"

__device__ inline double bessel_i0(double x) {
    double term = 1.0, sum = 1.0;
    const double q = 0.25 * x * x;
    for (int k = 1; k < 64; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

__device__ inline double resample_tap(int i, int L, int mpq, double beta) {
    const int half = (L - 1) / 2;
    const double r = (double)(i - half) / (double)half;
    const double kw = bessel_i0(beta * sqrt(fmax(0.0, 1.0 - r * r))) / bessel_i0(beta);
    const double x = (double)(i - half) / (double)mpq;
    const double s = i == half ? 1.0 : sinpi(x) / (M_PI * x);
    return kw * s / (double)mpq;
}

// the body of a taps kernel: launched as ONE workgroup of 256 threads
__device__ inline void resample_taps_body(int p, int mpq, int L, double beta, double* __restrict__ taps) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < L; i += 256) s += resample_tap(i, L, mpq, beta);
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double scale = (double)p / red[0];
    for (int i = tid; i < L; i += 256) taps[i] = resample_tap(i, L, mpq, beta) * scale;
}
