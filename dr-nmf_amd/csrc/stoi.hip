// STOI of compute_scores (score_audio.m:231, `stoi(xref, xest, fs_est)`) for a ragged batch on gfx950.
//
// The STOI toolbox (Taal et al., IEEE TASLP 19(7), 2011) is a third-party download of the reference
// (download_toolboxes.sh) and not in its tree: parity is pinned to the published algorithm only, as restated in
// include/drnmf_score.h and tests/stoi_ref.py [STOI-memory].  x = reference, y = estimate.  Six stages, each a
// kernel over the whole batch; every row is computed from its own samples alone, every sum in a fixed order, so
// a row's score is bitwise the same in any batch and in every run:
//   stoi_taps      Matlab resample's filter for p/q = 10000/fs reduced (L = 20 max(p,q) + 1 Kaiser(5)-windowed
//                  sinc taps, p h / sum h), fp64, one workgroup.
//   stoi_resample  y[m] = sum_k x[k] h[q m + (L-1)/2 - p k] for m < ceil(len p / q): one lane per output sample,
//                  all L taps in LDS (a lane reads every p-th: ~L/p = 32 taps at 16 kHz), fp64 fma in k order,
//                  stored as fp64.  Skipped at 10 kHz (the stages below then read the float32 input).
//   stoi_vad       one workgroup per signal: the energies of x's frames (hop 128, hanning(256), fp64, one wave
//                  per frame), their max, the keep mask e - max + 40 > 0 and the compaction index (kept frame c
//                  -> its frame of x) by a chunked exclusive scan in thread order.
//   stoi_band      one wave per band frame, 4 per workgroup.  Band frame i of the compacted signal is built on
//                  load from kept frames i-1, i, i+1 through the compaction index (the compacted signal is never
//                  written), windowed again and transformed as ONE 256-point complex FFT of its sample pairs
//                  (the real-input split and the radix-4 Stockham passes of csrc/stft.hip's fast path, in a
//                  wave-private LDS slice with no workgroup barrier) -- in fp64, as the resampled signal is
//                  kept: a band 80 dB below its frame's loudest keeps full relative precision, where fp32
//                  rounding of the samples or of the transform (~-140 dB of the frame) would cost it ~1e-3.  The
//                  epilogue sums |X_k|^2 over the 15 one-third-octave bands and stores sqrt as float32.
//   stoi_segment   one lane per (30-frame segment, band), fp64: alpha, the clipped Y', the centred correlation.
//   stoi_mean      one workgroup per signal: the fp64 mean of its segment scores in a fixed order.
// ESTOI (Jensen & Taal, IEEE/ACM TASLP 24(11), 2016; include/drnmf_estoi.h, tests/estoi_ref.py [ESTOI-memory]) is
// the same three first stages and another last step, through drnmf_stoi_ext:
//   estoi_segment  one wave per 30-frame segment: both 15 x 30 tiles in LDS as fp64, rows then columns centred and
//                  normalised, the 30 column products added in frame order.
//   estoi_mean     as stoi_mean, one value per segment.
// Plain arithmetic there too: a zero norm (a constant band, a silent stretch of the estimate) is 0 / 0 = NaN.
// The training criterion -STOI with its exact gradient (include/drnmf_stoi_loss.h, tests/stoi_loss_ref.py) is the same
// launches through drnmf_stoi_loss, then the stoi_loss_* kernels further down, which walk the stages backwards.
// Matlab edge semantics (not pystoi's): fewer than 30 band frames -> NaN; fmin ignores NaN, so a segment with
// sum Y^2 = 0 (alpha = inf, inf * 0 = NaN) takes Y' = X (1 + c) and scores 1; a zero-variance vector divides
// 0 by 0 and the NaN reaches the mean.
#include "common.h"
#include "resample_filter.h"
#include "../../include/drnmf_score.h"
#include "../../include/drnmf_estoi.h"
#include "../../include/drnmf_stoi_loss.h"

namespace {

constexpr int ST_FS = 10000, ST_N = 256, ST_HOP = 128, ST_J = 15, ST_SEG = 30;
constexpr int ST_MAX_PQ = 160;                     // L <= 3201 taps in LDS
constexpr int ST_LEN_CHUNK = 224;                  // lengths per upload launch (kernel-argument bytes)
constexpr double ST_CLIP = 1.0 + 5.6234132519034908;   // 1 + 10^(-beta/20), beta = -15 dB

// one-third-octave bands (fs 10 kHz, 512-point FFT, 150 Hz lowest centre): bins [lo, hi)
__constant__ int k_band_lo[ST_J] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174};
__constant__ int k_band_hi[ST_J] = {9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
constexpr int ST_K0 = 7, ST_K1 = 219;              // bins read by the bands
// The bands are contiguous, k_band_hi[j] == k_band_lo[j + 1], from ST_K0 = k_band_lo[0] to ST_K1 = k_band_hi[14]:
// stoi_loss_band_kernel finds a bin's band by counting the upper edges at or below it.

struct LenChunk {
    int64_t len[ST_LEN_CHUNK];
};

__device__ __forceinline__ int64_t resampled_len(int64_t len, int p, int q) {
    return (len * p + q - 1) / q;
}
__device__ __forceinline__ int vad_frames_dev(int64_t rlen) {
    return rlen >= ST_N + 1 ? (int)((rlen - ST_N - 1) / ST_HOP) + 1 : 0;
}
__device__ __forceinline__ double hanning256(int n) {      // Matlab hanning(256): 0.5 (1 - cos(2 pi (n+1) / 257))
    return 0.5 - 0.5 * cospi(2.0 * (double)(n + 1) / (double)(ST_N + 1));
}

// the caller's host lengths reach the device as kernel arguments: enqueued, no copy from pageable memory
__global__ void __launch_bounds__(256) stoi_lengths_kernel(LenChunk c, int n, int64_t* __restrict__ out) {
    const int i = threadIdx.x;
    if (i < n) out[i] = c.len[i];
}

// bessel_i0, resample_tap and the body of the taps kernel: resample_filter.h, shared with resample.hip
__global__ void __launch_bounds__(256) stoi_taps_kernel(int p, int mpq, int L, double* __restrict__ taps) {
    resample_taps_body(p, mpq, L, 5.0, taps);
}

// grid (ceil(max resampled length / 256), n_sig, 2): z = 0 the reference, 1 the estimate
__global__ void __launch_bounds__(256)
stoi_resample_kernel(const float* __restrict__ ref, const float* __restrict__ est, int64_t ld_in,
                     const int64_t* __restrict__ lens, int p, int q, int L, const double* __restrict__ taps,
                     double* __restrict__ xr, double* __restrict__ yr, int64_t ld_out) {
    extern __shared__ double h[];
    for (int i = threadIdx.x; i < L; i += 256) h[i] = taps[i];
    __syncthreads();
    const int sig = blockIdx.y;
    const int64_t len = lens[sig];
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= resampled_len(len, p, q)) return;
    const float* __restrict__ x = (blockIdx.z ? est : ref) + (size_t)sig * ld_in;
    double* __restrict__ y = (blockIdx.z ? yr : xr) + (size_t)sig * ld_out;
    const int64_t t0 = (int64_t)q * m + (L - 1) / 2;
    int64_t k1 = t0 / p;
    if (k1 > len - 1) k1 = len - 1;
    const int64_t lo = t0 - (L - 1);
    const int64_t k0 = lo <= 0 ? 0 : (lo + p - 1) / p;
    double acc = 0.0;
    for (int64_t k = k0; k <= k1; ++k) acc = fma((double)x[k], h[t0 - p * k], acc);
    y[m] = acc;
}

// one workgroup per signal; e [n_sig][V] fp64 frame energies (workspace), kidx [n_sig][V], nkept [n_sig].
// T: float (the input at 10 kHz) or double (resampled)
template <typename T>
__global__ void __launch_bounds__(256)
stoi_vad_kernel(const T* __restrict__ xr, int64_t ld, const int64_t* __restrict__ lens, int p, int q, int V,
                double* __restrict__ e, int* __restrict__ kidx, int* __restrict__ nkept,
                uint8_t* __restrict__ keep_out) {
    __shared__ double win[ST_N];
    __shared__ double red[256];
    __shared__ int cnt[256];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int sig = blockIdx.x;
    const int nv = vad_frames_dev(resampled_len(lens[sig], p, q));
    const T* __restrict__ x = xr + (size_t)sig * ld;
    double* __restrict__ es = e + (size_t)sig * V;
    win[tid] = hanning256(tid);
    __syncthreads();
    for (int j = wv; j < nv; j += 4) {
        const T* f = x + (int64_t)j * ST_HOP;
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double v = (double)f[lane + 64 * r] * win[lane + 64 * r];
            s = fma(v, v, s);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) es[j] = 20.0 * log10(sqrt(s) / 16.0);     // 16 = sqrt(256)
    }
    __syncthreads();
    double mx = -INFINITY;
    for (int j = tid; j < nv; j += 256) mx = fmax(mx, es[j]);
    red[tid] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
        __syncthreads();
    }
    const double emax = red[0];
    const int per = (nv + 255) / 256;
    const int j0 = tid * per < nv ? tid * per : nv;
    const int j1 = j0 + per < nv ? j0 + per : nv;
    int c = 0;
    for (int j = j0; j < j1; ++j) c += (es[j] - emax + 40.0) > 0.0;
    cnt[tid] = c;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) {
            const int v = cnt[t];
            cnt[t] = run;
            run += v;
        }
        nkept[sig] = run;
    }
    __syncthreads();
    int pos = cnt[tid];
    int* __restrict__ ki = kidx + (size_t)sig * V;
    for (int j = j0; j < j1; ++j) {
        const bool keep = (es[j] - emax + 40.0) > 0.0;
        if (keep) ki[pos++] = j;
        if (keep_out) keep_out[(size_t)sig * V + j] = keep;
    }
    if (keep_out)
        for (int j = nv + tid; j < V; j += 256) keep_out[(size_t)sig * V + j] = 0;
}

__device__ __forceinline__ double2 zmul(double2 a, double2 w) {
    return make_double2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

__device__ __forceinline__ void dft4(double2 (&v)[4]) {
    const double2 a = make_double2(v[0].x + v[2].x, v[0].y + v[2].y);
    const double2 b = make_double2(v[0].x - v[2].x, v[0].y - v[2].y);
    const double2 c = make_double2(v[1].x + v[3].x, v[1].y + v[3].y);
    const double2 d = make_double2(v[1].x - v[3].x, v[1].y - v[3].y);
    v[0] = make_double2(a.x + c.x, a.y + c.y);
    v[2] = make_double2(a.x - c.x, a.y - c.y);
    v[1] = make_double2(b.x + d.y, b.y - d.x);      // b - i d
    v[3] = make_double2(b.x - d.y, b.y + d.x);      // b + i d
}

// One wave's 256-point complex FFT (of the 512-point real frame's sample pairs) in its LDS slice
constexpr int FT_M = 256, FT_N = 512, FT_R = 4, FT_P = 4, FT_MP = FT_M + FT_M / 8;
__device__ __forceinline__ int ft_pad(int i) { return i + (i >> 3); }       // index i lives at i + i/8 (bank spread)

// sample t of compacted frame `frame`: the overlap-add of kept frames i (source start s0) and i -+ 1 (sp, sn),
// windowed again
template <typename T>
__device__ __forceinline__ double band_sample(const T* __restrict__ src, const double* win, int64_t s0, int64_t sp,
                                              int64_t sn, int frame, int t) {
    const double a = (double)src[s0 + t] * win[t];
    double b = 0.0;
    if (t < ST_HOP) {
        if (frame > 0) b = (double)src[sp + t + ST_HOP] * win[t + ST_HOP];
    } else {
        b = (double)src[sn + t - ST_HOP] * win[t - ST_HOP];
    }
    return (a + b) * win[t];
}

// The radix-4 Stockham passes: lane j enters with v[r] = z[j + 64 r] and the transform is left in buf (natural
// order, padded); tw = e^{-2 pi i k / 512}, k < 256.  Wave-private: fences and wave barriers only.
__device__ __forceinline__ void fft256_wave(double2 (&v)[FT_R], double2* buf, const double2* tw, int j) {
    constexpr int M = FT_M, N = FT_N, R = FT_R, P = FT_P;
    int Ns = 1;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        if (p > 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) v[r] = buf[ft_pad(j + r * (M / R))];
        }
        const int k = j & (Ns - 1);
        if (p > 0) {                       // twiddles e^{-2 pi i k r / (Ns R)}
            const int step = k * (N / (Ns * R));
#pragma unroll
            for (int r = 1; r < R; ++r) {
                const int idx = step * r;
                const double2 t = tw[idx & (N / 2 - 1)];
                v[r] = zmul(v[r], idx >= N / 2 ? make_double2(-t.x, -t.y) : t);
            }
        }
        dft4(v);
        const int j0 = (j - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) buf[ft_pad(j0 + r * Ns)] = v[r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        Ns *= R;
    }
}

// bin k of the real frame's spectrum from the packed transform in buf: X[k] = a - i w b
__device__ __forceinline__ double2 real_bin(const double2* buf, const double2* tw, int k) {
    const double2 zk = buf[ft_pad(k)];
    const double2 zc = buf[ft_pad(FT_M - k)];
    const double2 a = make_double2(0.5 * (zk.x + zc.x), 0.5 * (zk.y - zc.y));
    const double2 b = make_double2(0.5 * (zk.x - zc.x), 0.5 * (zk.y + zc.y));
    const double2 wb = zmul(b, tw[k]);
    return make_double2(a.x + wb.y, a.y - wb.x);
}

// grid (ceil(F / 4), n_sig), one wave per band frame; env [n_sig][F][15]
template <typename T>
__global__ void __launch_bounds__(256)
stoi_band_kernel(const T* __restrict__ xr, const T* __restrict__ yr, int64_t ld,
                 const int* __restrict__ kidx, const int* __restrict__ nkept, int V, int F,
                 float* __restrict__ env_x, float* __restrict__ env_y) {
    __shared__ double2 tw[FT_N / 2];           // e^{-2 pi i k / N}, k < N/2
    __shared__ double win[ST_N];
    __shared__ double2 bufs[4][FT_MP];         // per wave
    __shared__ double pw[4][ST_K1 - ST_K0];    // per wave: |X_k|^2 of the band bins
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    const int frame = blockIdx.x * 4 + wv, sig = blockIdx.y;
    {
        double sn, cs;
        sincospi(-2.0 * (double)tid / (double)FT_N, &sn, &cs);
        tw[tid] = make_double2(cs, sn);
        win[tid] = hanning256(tid);
    }
    __syncthreads();
    if (frame >= nkept[sig] - 1) return;       // (whole waves: no barrier below)
    const int* __restrict__ ki = kidx + (size_t)sig * V;
    const int64_t s0 = (int64_t)ki[frame] * ST_HOP;                        // kept frame i
    const int64_t sp = frame > 0 ? (int64_t)ki[frame - 1] * ST_HOP : 0;    // kept frame i - 1
    const int64_t sn = (int64_t)ki[frame + 1] * ST_HOP;                    // kept frame i + 1 (i < n_kept - 1)
    double2* buf = bufs[wv];
    for (int which = 0; which < 2; ++which) {
        const T* __restrict__ src = (which ? yr : xr) + (size_t)sig * ld;
        auto samp = [&](int t) { return band_sample(src, win, s0, sp, sn, frame, t); };
        // pass-0 input z[n] = (s[2n], s[2n+1]), n = j + 64 r; zero padding from n = 128 on
        double2 v[FT_R];
        v[0] = make_double2(samp(2 * j), samp(2 * j + 1));
        v[1] = make_double2(samp(2 * j + 128), samp(2 * j + 129));
        v[2] = make_double2(0.0, 0.0);
        v[3] = make_double2(0.0, 0.0);
        fft256_wave(v, buf, tw, j);
        // split the real spectrum of the band bins; |X_k|^2 to LDS
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = ST_K0 + j + 64 * i;
            if (k < ST_K1) {
                const double2 X = real_bin(buf, tw, k);
                pw[wv][k - ST_K0] = X.x * X.x + X.y * X.y;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (j < ST_J) {
            double acc = 0.0;
            for (int k = k_band_lo[j]; k < k_band_hi[j]; ++k) acc += pw[wv][k - ST_K0];
            float* __restrict__ env = which ? env_y : env_x;
            env[((size_t)sig * F + frame) * ST_J + j] = (float)sqrt(acc);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// One (segment, band) of step 4, shared by the score and by its gradient so that both take the same clip decisions.
// X, Y enter as the 30 envelopes of the reference and the estimate and leave centred, Y clipped first (Y').
struct SegStats {
    double alpha, sy, mx, my, nx, ny, rho;     // sqrt(Sx / Sy), Sy, the means of X and Y', the norms, the correlation
    unsigned u;                                // bit f: frame f is not clipped (alpha Y <= c X)
};
__device__ __forceinline__ SegStats segment_stats(double (&X)[ST_SEG], double (&Y)[ST_SEG]) {
    SegStats s;
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int f = 0; f < ST_SEG; ++f) {
        sx = fma(X[f], X[f], sx);
        sy = fma(Y[f], Y[f], sy);
    }
    const double alpha = sqrt(sx / sy);
    double mx = 0.0, my = 0.0;
    unsigned u = 0;
#pragma unroll
    for (int f = 0; f < ST_SEG; ++f) {
        const double ay = alpha * Y[f], cx = X[f] * ST_CLIP;
        if (ay <= cx) u |= 1u << f;
        Y[f] = fmin(ay, cx);                       // fmin: a NaN operand yields the other (Matlab min)
        mx += X[f];
        my += Y[f];
    }
    mx /= ST_SEG;
    my /= ST_SEG;
    double nx = 0.0, ny = 0.0;
#pragma unroll
    for (int f = 0; f < ST_SEG; ++f) {
        X[f] -= mx;
        Y[f] -= my;
        nx = fma(X[f], X[f], nx);
        ny = fma(Y[f], Y[f], ny);
    }
    nx = sqrt(nx);
    ny = sqrt(ny);
    double rho = 0.0;
#pragma unroll
    for (int f = 0; f < ST_SEG; ++f) rho = fma(X[f] / nx, Y[f] / ny, rho);
    s.alpha = alpha; s.sy = sy; s.mx = mx; s.my = my; s.nx = nx; s.ny = ny; s.rho = rho; s.u = u;
    return s;
}

// grid (ceil(S * 15 / 256), n_sig): lane g = segment * 15 + band; d [n_sig][S][15]
__global__ void __launch_bounds__(256)
stoi_segment_kernel(const float* __restrict__ env_x, const float* __restrict__ env_y,
                    const int* __restrict__ nkept, int F, int S, double* __restrict__ d) {
    const int sig = blockIdx.y;
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int seg = g / ST_J, band = g - seg * ST_J;
    if (seg >= nkept[sig] - 1 - (ST_SEG - 1)) return;
    const float* __restrict__ ex = env_x + ((size_t)sig * F + seg) * ST_J + band;
    const float* __restrict__ ey = env_y + ((size_t)sig * F + seg) * ST_J + band;
    double X[ST_SEG], Y[ST_SEG];
#pragma unroll
    for (int f = 0; f < ST_SEG; ++f) {
        X[f] = (double)ex[f * ST_J];
        Y[f] = (double)ey[f * ST_J];
    }
    d[(size_t)sig * S * ST_J + g] = segment_stats(X, Y).rho;
}

// the fp64 mean of ds[0 .. cnt) by one workgroup, in a fixed order (cnt > 0)
__device__ __forceinline__ void mean_fixed_order(const double* __restrict__ ds, int cnt, double (&red)[256],
                                                 float* __restrict__ out) {
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int g = tid; g < cnt; g += 256) s += ds[g];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) *out = (float)(red[0] / (double)cnt);
}

__global__ void __launch_bounds__(256)
stoi_mean_kernel(const double* __restrict__ d, const int* __restrict__ nkept, int S, float* __restrict__ out) {
    __shared__ double red[256];
    const int sig = blockIdx.x;
    const int nseg = nkept[sig] - 1 - (ST_SEG - 1);
    if (nseg <= 0) {                           // Matlab's mean of an empty set
        if (threadIdx.x == 0) out[sig] = __int_as_float(0x7fc00000);
        return;
    }
    mean_fixed_order(d + (size_t)sig * S * ST_J, nseg * ST_J, red, out + sig);
}

// ESTOI's last step (include/drnmf_estoi.h, step 4'): grid (ceil(S / 4), n_sig), one wave per 30-frame segment, 4 per
// workgroup; d [n_sig][S].  The wave stages its two 15 x 30 tiles (band by frame) as fp64 in a wave-private LDS
// slice, normalises the rows with one lane per (tile, band), then the columns with one lane per frame, and lane 0
// adds the 30 column terms in frame order.  No workgroup barrier: whole waves leave at the top.
__global__ void __launch_bounds__(256)
estoi_segment_kernel(const float* __restrict__ env_x, const float* __restrict__ env_y,
                     const int* __restrict__ nkept, int F, int S, double* __restrict__ d) {
    constexpr int TILE = ST_J * ST_SEG;
    __shared__ double tiles[4][2][TILE];       // [wave][x, y][band * 30 + frame]
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int sig = blockIdx.y, seg = blockIdx.x * 4 + wv;
    if (seg >= nkept[sig] - 1 - (ST_SEG - 1)) return;
    double* tx = tiles[wv][0];
    double* ty = tiles[wv][1];
    // frames seg .. seg + 29 are 450 consecutive floats of each envelope
    const float* __restrict__ ex = env_x + ((size_t)sig * F + seg) * ST_J;
    const float* __restrict__ ey = env_y + ((size_t)sig * F + seg) * ST_J;
    for (int i = lane; i < TILE; i += 64) {
        const int f = i / ST_J, b = i - f * ST_J;
        tx[b * ST_SEG + f] = (double)ex[i];
        ty[b * ST_SEG + f] = (double)ey[i];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // rows: lanes 0-14 the bands of x, lanes 32-46 the bands of y
    if ((lane & 31) < ST_J) {
        double* row = tiles[wv][lane >> 5] + (lane & 31) * ST_SEG;
        double a[ST_SEG];
        double m = 0.0;
#pragma unroll
        for (int f = 0; f < ST_SEG; ++f) {
            a[f] = row[f];
            m += a[f];
        }
        m /= ST_SEG;
        double n = 0.0;
#pragma unroll
        for (int f = 0; f < ST_SEG; ++f) {
            a[f] -= m;
            n = fma(a[f], a[f], n);
        }
        n = sqrt(n);
#pragma unroll
        for (int f = 0; f < ST_SEG; ++f) row[f] = a[f] / n;      // a constant band: 0 / 0 = NaN
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // columns: lane f normalises frame f of both tiles and multiplies them
    double term = 0.0;
    if (lane < ST_SEG) {
        double x[ST_J], y[ST_J];
        double mx = 0.0, my = 0.0;
#pragma unroll
        for (int b = 0; b < ST_J; ++b) {
            x[b] = tx[b * ST_SEG + lane];
            y[b] = ty[b * ST_SEG + lane];
            mx += x[b];
            my += y[b];
        }
        mx /= ST_J;
        my /= ST_J;
        double nx = 0.0, ny = 0.0;
#pragma unroll
        for (int b = 0; b < ST_J; ++b) {
            x[b] -= mx;
            y[b] -= my;
            nx = fma(x[b], x[b], nx);
            ny = fma(y[b], y[b], ny);
        }
        nx = sqrt(nx);
        ny = sqrt(ny);
#pragma unroll
        for (int b = 0; b < ST_J; ++b) term = fma(x[b] / nx, y[b] / ny, term);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();           // every lane has read its column: tx is free
    if (lane < ST_SEG) tx[lane] = term;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        double acc = 0.0;
#pragma unroll
        for (int f = 0; f < ST_SEG; ++f) acc += tx[f];
        d[(size_t)sig * S + seg] = acc / ST_SEG;
    }
}

__global__ void __launch_bounds__(256)
estoi_mean_kernel(const double* __restrict__ d, const int* __restrict__ nkept, int S, float* __restrict__ out) {
    __shared__ double red[256];
    const int sig = blockIdx.x;
    const int nseg = nkept[sig] - 1 - (ST_SEG - 1);
    if (nseg <= 0) {                           // as STOI: the mean of an empty set
        if (threadIdx.x == 0) out[sig] = __int_as_float(0x7fc00000);
        return;
    }
    mean_fixed_order(d + (size_t)sig * S, nseg, red, out + sig);
}

// ---- the gradient of -STOI with respect to the estimate (include/drnmf_stoi_loss.h) ----------------------------
// The forward's stages walked backwards, fp64 throughout, every sum a gather in a fixed order (no atomics): a row's
// gradient is bitwise the same in any batch and in every run.  The silence decision and the compaction index depend
// on the reference only, so nothing flows through them.
//   stoi_loss_rows      one workgroup: loss = -STOI and counted = 1 where STOI is finite (0, 0 elsewhere), sums[2].
//   stoi_loss_seg       one lane per (segment, band), the arithmetic of stoi_segment_kernel (the same clip
//                       decisions u: the shared segment_stats), then the segment's scalars: alpha, c2 = (1/Sy) sum_u g Y', the two means and
//                       inverse norms and d, with g = (x^ - d y^) / ||Y' - mean||.
//   stoi_loss_env       one lane per (band frame, band): gY = -1/(S J) sum over the <= 30 segments that hold the
//                       frame of alpha u g - c2 Y; a segment with Sy == 0 adds nothing.
//   stoi_loss_band      one wave per band frame: the estimate's frame transformed as stoi_band_kernel does, the
//                       band bins scaled by gY / Y (0 where Y == 0), and the adjoint w[n] Re sum_k G_k e^{+2 pi i k
//                       n / 512} through the same passes: the Hermitian extension of G folded into a 256-point
//                       complex inverse, run as the conjugate of the forward transform of the conjugate.
//   stoi_loss_gather    one lane per 10 kHz sample: its <= 2 silence-detector frames, each found in the compaction
//                       index by bisection, each gathering its <= 2 band frames.  At 10 kHz this writes g.
//   stoi_loss_resample  one lane per input sample: the transposed polyphase filter, the taps in LDS.
constexpr int SL_SEG_W = 7;        // doubles per (segment, band): alpha (< 0: no gradient), c2, mx, 1/nx, my, 1/ny, d

__global__ void __launch_bounds__(256)
stoi_loss_rows_kernel(const float* __restrict__ stoi, int n_sig, float* __restrict__ loss,
                      float* __restrict__ counted, float* __restrict__ sums) {
    __shared__ double s0[256], s1[256];
    double tot = 0.0, cnt = 0.0;
    for (int row = threadIdx.x; row < n_sig; row += 256) {
        const float s = stoi[row];
        const bool on = isfinite(s);
        const float l = on ? -s : 0.f;
        loss[row] = l;
        counted[row] = on ? 1.f : 0.f;
        if (on) {
            tot += (double)l;
            cnt += 1.0;
        }
    }
    s0[threadIdx.x] = tot;
    s1[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s0[threadIdx.x] += s0[threadIdx.x + o];
            s1[threadIdx.x] += s1[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sums[0] = (float)s0[0];
        sums[1] = (float)s1[0];
    }
}

// grid as stoi_segment_kernel; sb [n_sig][S][15][SL_SEG_W]
__global__ void __launch_bounds__(256)
stoi_loss_seg_kernel(const float* __restrict__ env_x, const float* __restrict__ env_y,
                     const int* __restrict__ nkept, int F, int S, double* __restrict__ sb) {
    const int sig = blockIdx.y;
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int seg = g / ST_J, band = g - seg * ST_J;
    if (seg >= nkept[sig] - 1 - (ST_SEG - 1)) return;
    const float* __restrict__ ex = env_x + ((size_t)sig * F + seg) * ST_J + band;
    const float* __restrict__ ey = env_y + ((size_t)sig * F + seg) * ST_J + band;
    double X[ST_SEG], Y[ST_SEG];
#pragma unroll
    for (int f = 0; f < ST_SEG; ++f) {
        X[f] = (double)ex[f * ST_J];
        Y[f] = (double)ey[f * ST_J];
    }
    const SegStats st = segment_stats(X, Y);
    const double nx = st.nx, ny = st.ny, rho = st.rho, my = st.my;
    const unsigned u = st.u;
    // sum over the unclipped frames of g Y', Y' = alpha Y there
    double acc = 0.0;
#pragma unroll
    for (int f = 0; f < ST_SEG; ++f) {
        const double gf = (X[f] / nx - rho * (Y[f] / ny)) / ny;
        if ((u >> f) & 1u) acc = fma(gf, Y[f] + my, acc);
    }
    double* __restrict__ o = sb + ((size_t)sig * S * ST_J + g) * SL_SEG_W;
    o[0] = st.sy > 0.0 ? st.alpha : -1.0;          // Sy == 0: scored 1, no gradient
    o[1] = acc / st.sy;
    o[2] = st.mx;
    o[3] = 1.0 / nx;
    o[4] = my;
    o[5] = 1.0 / ny;
    o[6] = rho;
}

// grid (ceil(F * 15 / 256), n_sig): lane e = band frame * 15 + band; gy [n_sig][F][15]
__global__ void __launch_bounds__(256)
stoi_loss_env_kernel(const float* __restrict__ env_x, const float* __restrict__ env_y,
                     const int* __restrict__ nkept, int F, int S, const double* __restrict__ sb,
                     double* __restrict__ gy) {
    const int sig = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int frame = e / ST_J, band = e - frame * ST_J;
    const int nf = nkept[sig] - 1, nseg = nf - (ST_SEG - 1);
    if (nseg <= 0 || frame >= nf) return;
    const double X = (double)env_x[(size_t)sig * F * ST_J + e];
    const double Y = (double)env_y[(size_t)sig * F * ST_J + e];
    const double cx = X * ST_CLIP;
    const int m0 = frame - (ST_SEG - 1) > 0 ? frame - (ST_SEG - 1) : 0;
    const int m1 = frame < nseg - 1 ? frame : nseg - 1;
    double acc = 0.0;
    for (int m = m0; m <= m1; ++m) {
        const double* __restrict__ s = sb + (((size_t)sig * S + m) * ST_J + band) * SL_SEG_W;
        const double alpha = s[0];
        if (!(alpha >= 0.0)) continue;
        const double ay = alpha * Y;
        double t = -s[1] * Y;
        if (ay <= cx) {
            const double xh = (X - s[2]) * s[3], yh = (ay - s[4]) * s[5];
            t = fma(alpha, (xh - s[6] * yh) * s[5], t);
        }
        acc += t;
    }
    gy[(size_t)sig * F * ST_J + e] = -acc / ((double)nseg * ST_J);
}

// grid as stoi_band_kernel, one wave per band frame; fr [n_sig][F][256]: the gradient with respect to the frame's
// samples of the compacted estimate
template <typename T>
__global__ void __launch_bounds__(256)
stoi_loss_band_kernel(const T* __restrict__ yr, int64_t ld, const int* __restrict__ kidx,
                      const int* __restrict__ nkept, int V, int F, const double* __restrict__ gy,
                      double* __restrict__ fr) {
    constexpr int NB = ST_K1 - ST_K0;
    __shared__ double2 tw[FT_N / 2];
    __shared__ double win[ST_N];
    __shared__ double2 bufs[4][FT_MP];
    __shared__ double2 zs[4][NB];              // per wave: the band bins Z_k, then G_k
    __shared__ double sc[4][16];               // per wave: gY / Y of the 15 bands
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    const int frame = blockIdx.x * 4 + wv, sig = blockIdx.y;
    {
        double sn, cs;
        sincospi(-2.0 * (double)tid / (double)FT_N, &sn, &cs);
        tw[tid] = make_double2(cs, sn);
        win[tid] = hanning256(tid);
    }
    __syncthreads();
    const int nf = nkept[sig] - 1;
    if (nf < ST_SEG || frame >= nf) return;    // (whole waves: no barrier below)
    const int* __restrict__ ki = kidx + (size_t)sig * V;
    const int64_t s0 = (int64_t)ki[frame] * ST_HOP;
    const int64_t sp = frame > 0 ? (int64_t)ki[frame - 1] * ST_HOP : 0;
    const int64_t sn = (int64_t)ki[frame + 1] * ST_HOP;
    const T* __restrict__ src = yr + (size_t)sig * ld;
    double2* buf = bufs[wv];
    double2* z = zs[wv];
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    double2 v[FT_R];
    v[0] = make_double2(band_sample(src, win, s0, sp, sn, frame, 2 * j),
                        band_sample(src, win, s0, sp, sn, frame, 2 * j + 1));
    v[1] = make_double2(band_sample(src, win, s0, sp, sn, frame, 2 * j + 128),
                        band_sample(src, win, s0, sp, sn, frame, 2 * j + 129));
    v[2] = make_double2(0.0, 0.0);
    v[3] = make_double2(0.0, 0.0);
    fft256_wave(v, buf, tw, j);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = ST_K0 + j + 64 * i;
        if (k < ST_K1) z[k - ST_K0] = real_bin(buf, tw, k);
    }
    wave_sync();
    if (j < ST_J) {
        double acc = 0.0;
        for (int k = k_band_lo[j]; k < k_band_hi[j]; ++k) {
            const double2 a = z[k - ST_K0];
            acc += a.x * a.x + a.y * a.y;
        }
        const double Y = sqrt(acc);
        sc[wv][j] = Y > 0.0 ? gy[((size_t)sig * F + frame) * ST_J + j] / Y : 0.0;
    }
    wave_sync();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = ST_K0 + j + 64 * i;
        if (k < ST_K1) {
            int b = 0;                         // the bands are contiguous: count the upper edges at or below k
#pragma unroll
            for (int t = 0; t < ST_J - 1; ++t) b += k >= k_band_hi[t];
            const double s = sc[wv][b];
            const double2 a = z[k - ST_K0];
            z[k - ST_K0] = make_double2(a.x * s, a.y * s);
        }
    }
    wave_sync();
    // r[n] = Re sum_k G_k e^{+2 pi i k n / 512} = sum over the Hermitian extension H (H_k = G_k / 2, H_{512-k} its
    // conjugate); with r packed as r[2m] + i r[2m+1] = sum_{k < 256} Q_k e^{+2 pi i k m / 256},
    // Q_k = (H_k + H_{k+256}) + i e^{+2 pi i k / 512} (H_k - H_{k+256}).  The passes transform conj(Q).
#pragma unroll
    for (int r = 0; r < FT_R; ++r) {
        const int k = j + 64 * r, kc = FT_M - k;
        const double2 ha = k >= ST_K0 && k < ST_K1 ? z[k - ST_K0] : make_double2(0.0, 0.0);
        double2 hb = kc >= ST_K0 && kc < ST_K1 ? z[kc - ST_K0] : make_double2(0.0, 0.0);
        hb.y = -hb.y;
        const double2 t = tw[k];
        const double2 ed = zmul(make_double2(ha.x - hb.x, ha.y - hb.y), make_double2(t.x, -t.y));
        v[r] = make_double2(0.5 * (ha.x + hb.x - ed.y), -0.5 * (ha.y + hb.y + ed.x));
    }
    wave_sync();                               // every lane has read z and buf
    fft256_wave(v, buf, tw, j);
    double2* __restrict__ out = (double2*)(fr + ((size_t)sig * F + frame) * ST_N);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = j + 64 * i;
        const double2 a = buf[ft_pad(m)];      // conj(r[2m] + i r[2m+1])
        out[m] = make_double2(win[2 * m] * a.x, -win[2 * m + 1] * a.y);
    }
}

// grid (ceil(width / 256), n_sig): sample m of the 10 kHz estimate.  O = double: the resampled signal's gradient
// gr [n_sig][ld_out]; O = float: g itself (fs = 10 kHz), zeros behind the length and in a row that is not counted.
template <typename O>
__global__ void __launch_bounds__(256)
stoi_loss_gather_kernel(const double* __restrict__ fr, const int* __restrict__ kidx,
                        const int* __restrict__ nkept, const int64_t* __restrict__ lens,
                        const float* __restrict__ stoi, int p, int q, int V, int F, int64_t width,
                        O* __restrict__ out, int64_t ld_out) {
    __shared__ double win[ST_N];
    win[threadIdx.x] = hanning256(threadIdx.x);
    __syncthreads();
    const int sig = blockIdx.y;
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= width) return;
    const int64_t rlen = resampled_len(lens[sig], p, q);
    const int nk = nkept[sig], nf = nk - 1;
    double acc = 0.0;
    if (m < rlen && nf >= ST_SEG && isfinite(stoi[sig])) {
        const int nv = vad_frames_dev(rlen);
        const int* __restrict__ ki = kidx + (size_t)sig * V;
        const double* __restrict__ f = fr + (size_t)sig * F * ST_N;
        const int jhi = (int)(m >> 7);
        for (int jj = jhi - 1; jj <= jhi; ++jj) {
            if (jj < 0 || jj >= nv) continue;
            int lo = 0, hi = nk;               // the kept index of silence-detector frame jj, if it was kept
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (ki[mid] < jj) lo = mid + 1; else hi = mid;
            }
            if (lo >= nk || ki[lo] != jj) continue;
            const int n = (int)(m - (int64_t)jj * ST_HOP);
            const int i1 = lo + (n >> 7), t = n & (ST_HOP - 1);
            double gys = 0.0;                  // compacted sample 128 lo + n: band frames i1 - 1 and i1
            if (i1 >= 1 && i1 - 1 < nf) gys += f[(size_t)(i1 - 1) * ST_N + t + ST_HOP];
            if (i1 < nf) gys += f[(size_t)i1 * ST_N + t];
            acc = fma(win[n], gys, acc);
        }
    }
    out[(size_t)sig * ld_out + m] = (O)acc;
}

// grid (ceil(stride / 256), n_sig): g[k] = sum_m gr[m] h[q m + (L-1)/2 - p k] in m order, 0 behind the length and
// in a row that is not counted
__global__ void __launch_bounds__(256)
stoi_loss_resample_kernel(const double* __restrict__ gr, int64_t ld_r, const int64_t* __restrict__ lens,
                          const float* __restrict__ stoi, int p, int q, int L, const double* __restrict__ taps,
                          float* __restrict__ g, int64_t stride) {
    extern __shared__ double h[];
    for (int i = threadIdx.x; i < L; i += 256) h[i] = taps[i];
    __syncthreads();
    const int sig = blockIdx.y;
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= stride) return;
    const int64_t len = lens[sig];
    double acc = 0.0;
    if (k < len && isfinite(stoi[sig])) {
        const int64_t half = (L - 1) / 2, lo = (int64_t)p * k - half;
        const int64_t m0 = lo <= 0 ? 0 : (lo + q - 1) / q;
        int64_t m1 = ((int64_t)p * k + half) / q;
        const int64_t rlen = resampled_len(len, p, q);
        if (m1 > rlen - 1) m1 = rlen - 1;
        const double* __restrict__ x = gr + (size_t)sig * ld_r;
        for (int64_t m = m0; m <= m1; ++m) acc = fma(x[m], h[q * m - lo], acc);
    }
    g[(size_t)sig * stride + k] = (float)acc;
}

int gcd_i(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// p / q = 10000 / fs reduced; false when unsupported
bool stoi_rate(int32_t fs, int& p, int& q) {
    if (fs <= 0) return false;
    const int g = gcd_i(ST_FS, fs);
    p = ST_FS / g;
    q = fs / g;
    return (p > q ? p : q) <= ST_MAX_PQ;
}

int64_t resampled_len_h(int64_t len, int p, int q) { return (len * p + q - 1) / q; }
int vad_frames_h(int64_t rlen) { return rlen >= ST_N + 1 ? (int)((rlen - ST_N - 1) / ST_HOP) + 1 : 0; }

struct StoiLayout {
    int p, q, mpq, L;
    bool rs;                 // resample (fs != 10 kHz)
    int64_t rstride;         // row stride of the resampled signals
    int V, F, S;             // VAD frames, band frames (>= 1), segments (>= 1) bounds
    size_t off_len, off_taps, off_xr, off_yr, off_e, off_kidx, off_nk, off_envx, off_envy, off_d, total;
};

constexpr int64_t ST_MAX_LEN = (int64_t)1 << 30;

bool stoi_layout(int32_t n_sig, int64_t max_len, int32_t fs, StoiLayout& Lo) {
    if (n_sig <= 0 || max_len < 0 || max_len > ST_MAX_LEN || !stoi_rate(fs, Lo.p, Lo.q)) return false;
    Lo.mpq = Lo.p > Lo.q ? Lo.p : Lo.q;
    Lo.rs = Lo.p != Lo.q;
    Lo.L = 20 * Lo.mpq + 1;
    const int64_t rmax = resampled_len_h(max_len, Lo.p, Lo.q);
    Lo.rstride = rmax < 64 ? 64 : (int64_t)round_up_sz((size_t)rmax, 64);
    Lo.V = vad_frames_h(rmax);
    Lo.F = Lo.V > 1 ? Lo.V - 1 : 1;
    Lo.S = Lo.F > ST_SEG - 1 ? Lo.F - (ST_SEG - 1) : 1;
    const size_t n = (size_t)n_sig;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += round_up_sz(bytes, 256);
        return at;
    };
    Lo.off_len = take(n * sizeof(int64_t));
    Lo.off_taps = take(Lo.rs ? (size_t)Lo.L * sizeof(double) : 0);
    Lo.off_xr = take(Lo.rs ? n * Lo.rstride * sizeof(double) : 0);
    Lo.off_yr = take(Lo.rs ? n * Lo.rstride * sizeof(double) : 0);
    Lo.off_e = take(n * (Lo.V > 0 ? Lo.V : 1) * sizeof(double));
    Lo.off_kidx = take(n * (Lo.V > 0 ? Lo.V : 1) * sizeof(int));
    Lo.off_nk = take(n * sizeof(int));
    Lo.off_envx = take(n * Lo.F * ST_J * sizeof(float));
    Lo.off_envy = take(n * Lo.F * ST_J * sizeof(float));
    Lo.off_d = take(n * Lo.S * ST_J * sizeof(double));
    Lo.total = o;
    return true;
}

}  // namespace

extern "C" int32_t drnmf_stoi_vad_frames(int64_t len, int32_t fs) {
    int p, q;
    if (len < 0 || len > ST_MAX_LEN || !stoi_rate(fs, p, q)) return -1;
    return vad_frames_h(resampled_len_h(len, p, q));
}

extern "C" size_t drnmf_stoi_workspace_bytes(int32_t n_sig, int64_t max_len, int32_t fs) {
    StoiLayout Lo;
    return stoi_layout(n_sig, max_len, fs, Lo) ? Lo.total : 0;
}

namespace {

// what steps 1 to 3 leave on the device for the last step of either score
struct StoiFront {
    const int* nk;           // [n_sig] kept frames
    const float* envx;       // [n_sig][F][15] band envelopes of the reference ...
    const float* envy;       // ... and of the estimate
};

// The checks of drnmf_stoi and drnmf_stoi_ext (`who` names the caller in the message); fills Lo and max_len.
int32_t stoi_check(drnmf_handle_t h, const char* who, int32_t n_sig, int64_t stride, const int64_t* lengths_host,
                   int32_t fs, const float* est, const float* ref, bool have_out, bool have_ws, StoiLayout& Lo,
                   int64_t& max_len) {
    if (n_sig <= 0 || n_sig > 65535 || stride <= 0 || !lengths_host || !est || !ref || !have_out || !have_ws)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: bad argument (n_sig in [1, 65535], stride > 0, non-NULL)", who);
    max_len = 0;
    for (int i = 0; i < n_sig; ++i) {
        const int64_t l = lengths_host[i];
        if (l < 0 || l > stride || l > ST_MAX_LEN)
            DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: lengths[%d] = %lld outside [0, min(stride, 2^30)]", who, i,
                       (long long)l);
        if (l > max_len) max_len = l;
    }
    if (!stoi_layout(n_sig, max_len, fs, Lo))
        DRNMF_FAIL(h, DRNMF_ERR_UNSUPPORTED,
                   "%s: fs = %d unsupported (10000/fs reduced to p/q must have max(p, q) <= 160)", who, fs);
    return DRNMF_OK;
}

// Steps 1 to 3: lengths, resampling, the silence decision and the band envelopes of the whole batch.
StoiFront stoi_front(const StoiLayout& Lo, int32_t n_sig, int64_t stride, const int64_t* lengths_host,
                     int64_t max_len, const float* est, const float* ref, uint8_t* keep_out, float* env_ref_out,
                     float* env_est_out, char* ws, hipStream_t stream) {
    int64_t* lens = (int64_t*)(ws + Lo.off_len);
    for (int base = 0; base < n_sig; base += ST_LEN_CHUNK) {
        LenChunk c;
        const int n = n_sig - base < ST_LEN_CHUNK ? n_sig - base : ST_LEN_CHUNK;
        for (int i = 0; i < ST_LEN_CHUNK; ++i) c.len[i] = i < n ? lengths_host[base + i] : 0;
        hipLaunchKernelGGL(stoi_lengths_kernel, dim3(1), dim3(256), 0, stream, c, n, lens + base);
    }
    double* e = (double*)(ws + Lo.off_e);
    int* kidx = (int*)(ws + Lo.off_kidx);
    int* nk = (int*)(ws + Lo.off_nk);
    float* envx = env_ref_out ? env_ref_out : (float*)(ws + Lo.off_envx);
    float* envy = env_est_out ? env_est_out : (float*)(ws + Lo.off_envy);
    const int V = Lo.V > 0 ? Lo.V : 1;
    uint8_t* keep = Lo.V > 0 ? keep_out : nullptr;
    const dim3 band_grid((unsigned)((Lo.F + 3) / 4), (unsigned)n_sig);
    if (Lo.rs) {
        double* taps = (double*)(ws + Lo.off_taps);
        double* xr = (double*)(ws + Lo.off_xr);
        double* yr = (double*)(ws + Lo.off_yr);
        hipLaunchKernelGGL(stoi_taps_kernel, dim3(1), dim3(256), 0, stream, Lo.p, Lo.mpq, Lo.L, taps);
        const unsigned nb = (unsigned)((resampled_len_h(max_len, Lo.p, Lo.q) + 255) / 256);
        hipLaunchKernelGGL(stoi_resample_kernel, dim3(nb > 0 ? nb : 1, (unsigned)n_sig, 2), dim3(256),
                           (size_t)Lo.L * sizeof(double), stream, ref, est, stride, (const int64_t*)lens, Lo.p,
                           Lo.q, Lo.L, (const double*)taps, xr, yr, Lo.rstride);
        hipLaunchKernelGGL(stoi_vad_kernel<double>, dim3((unsigned)n_sig), dim3(256), 0, stream,
                           (const double*)xr, Lo.rstride, (const int64_t*)lens, Lo.p, Lo.q, V, e, kidx, nk, keep);
        hipLaunchKernelGGL(stoi_band_kernel<double>, band_grid, dim3(256), 0, stream, (const double*)xr,
                           (const double*)yr, Lo.rstride, (const int*)kidx, (const int*)nk, V, Lo.F, envx, envy);
    } else {
        hipLaunchKernelGGL(stoi_vad_kernel<float>, dim3((unsigned)n_sig), dim3(256), 0, stream, ref, stride,
                           (const int64_t*)lens, Lo.p, Lo.q, V, e, kidx, nk, keep);
        hipLaunchKernelGGL(stoi_band_kernel<float>, band_grid, dim3(256), 0, stream, ref, est, stride,
                           (const int*)kidx, (const int*)nk, V, Lo.F, envx, envy);
    }
    return StoiFront{nk, envx, envy};
}

// STOI's step 4 and its mean
void stoi_back(const StoiLayout& Lo, int32_t n_sig, const StoiFront& fr, float* stoi_out, char* ws,
               hipStream_t stream) {
    double* d = (double*)(ws + Lo.off_d);
    hipLaunchKernelGGL(stoi_segment_kernel, dim3((unsigned)((Lo.S * ST_J + 255) / 256), (unsigned)n_sig),
                       dim3(256), 0, stream, fr.envx, fr.envy, fr.nk, Lo.F, Lo.S, d);
    hipLaunchKernelGGL(stoi_mean_kernel, dim3((unsigned)n_sig), dim3(256), 0, stream, (const double*)d, fr.nk,
                       Lo.S, stoi_out);
}

// drnmf_stoi_ext's workspace: drnmf_stoi's, then the per-segment ESTOI scores d [n_sig][S] fp64
size_t estoi_d_bytes(const StoiLayout& Lo, int32_t n_sig) {
    return round_up_sz((size_t)n_sig * Lo.S * sizeof(double), 256);
}

}  // namespace

extern "C" int32_t drnmf_stoi(drnmf_handle_t h, int32_t n_sig, int64_t stride, const int64_t* lengths_host,
                              int32_t fs, const float* est, const float* ref, float* stoi_out, uint8_t* keep_out,
                              float* env_ref_out, float* env_est_out, void* workspace, size_t workspace_bytes,
                              void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    StoiLayout Lo;
    int64_t max_len;
    const int32_t rc = stoi_check(h, "stoi", n_sig, stride, lengths_host, fs, est, ref, stoi_out != nullptr,
                                  workspace != nullptr, Lo, max_len);
    if (rc != DRNMF_OK) return rc;
    if (workspace_bytes < Lo.total)
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "stoi: workspace too small (%zu < %zu bytes)", workspace_bytes,
                   Lo.total);
    hipStream_t stream = (hipStream_t)stream_;
    const StoiFront fr = stoi_front(Lo, n_sig, stride, lengths_host, max_len, est, ref, keep_out, env_ref_out,
                                    env_est_out, (char*)workspace, stream);
    stoi_back(Lo, n_sig, fr, stoi_out, (char*)workspace, stream);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

extern "C" size_t drnmf_stoi_ext_workspace_bytes(int32_t n_sig, int64_t max_len, int32_t fs) {
    StoiLayout Lo;
    return stoi_layout(n_sig, max_len, fs, Lo) ? Lo.total + estoi_d_bytes(Lo, n_sig) : 0;
}

extern "C" int32_t drnmf_stoi_ext(drnmf_handle_t h, int32_t n_sig, int64_t stride, const int64_t* lengths_host,
                                  int32_t fs, const float* est, const float* ref, float* stoi_out, float* estoi_out,
                                  uint8_t* keep_out, float* env_ref_out, float* env_est_out, double* d_ext_out,
                                  void* workspace, size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    StoiLayout Lo;
    int64_t max_len;
    const int32_t rc = stoi_check(h, "stoi_ext", n_sig, stride, lengths_host, fs, est, ref,
                                  stoi_out != nullptr || estoi_out != nullptr, workspace != nullptr, Lo, max_len);
    if (rc != DRNMF_OK) return rc;
    const size_t need = Lo.total + estoi_d_bytes(Lo, n_sig);
    if (workspace_bytes < need)
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "stoi_ext: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    if (((uintptr_t)workspace & 255) != 0)
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "stoi_ext: workspace is not 256-byte aligned");
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "stoi_ext: the handle is bound to no device");
    hipStream_t stream = (hipStream_t)stream_;
    const StoiFront fr = stoi_front(Lo, n_sig, stride, lengths_host, max_len, est, ref, keep_out, env_ref_out,
                                    env_est_out, (char*)workspace, stream);
    if (stoi_out) stoi_back(Lo, n_sig, fr, stoi_out, (char*)workspace, stream);
    if (estoi_out || d_ext_out) {
        double* d = d_ext_out ? d_ext_out : (double*)((char*)workspace + Lo.total);
        hipLaunchKernelGGL(estoi_segment_kernel, dim3((unsigned)((Lo.S + 3) / 4), (unsigned)n_sig), dim3(256), 0,
                           stream, fr.envx, fr.envy, fr.nk, Lo.F, Lo.S, d);
        if (estoi_out)
            hipLaunchKernelGGL(estoi_mean_kernel, dim3((unsigned)n_sig), dim3(256), 0, stream, (const double*)d,
                               fr.nk, Lo.S, estoi_out);
    }
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

namespace {

// drnmf_stoi_loss's workspace: drnmf_stoi's, then the scores, the segment scalars, gY, the frame gradients and
// (fs != 10 kHz) the gradient of the resampled estimate
struct StoiLossLayout {
    size_t off_stoi, off_sb, off_gy, off_fr, off_gr, total;
};

StoiLossLayout stoi_loss_layout(const StoiLayout& Lo, int32_t n_sig) {
    StoiLossLayout G;
    const size_t n = (size_t)n_sig;
    size_t o = Lo.total;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += round_up_sz(bytes, 256);
        return at;
    };
    G.off_stoi = take(n * sizeof(float));
    G.off_sb = take(n * Lo.S * ST_J * SL_SEG_W * sizeof(double));
    G.off_gy = take(n * Lo.F * ST_J * sizeof(double));
    G.off_fr = take(n * Lo.F * ST_N * sizeof(double));
    G.off_gr = take(Lo.rs ? n * Lo.rstride * sizeof(double) : 0);
    G.total = o;
    return G;
}

}  // namespace

extern "C" size_t drnmf_stoi_loss_workspace_bytes(int32_t n_sig, int64_t max_len, int32_t fs) {
    StoiLayout Lo;
    return stoi_layout(n_sig, max_len, fs, Lo) ? stoi_loss_layout(Lo, n_sig).total : 0;
}

extern "C" int32_t drnmf_stoi_loss(drnmf_handle_t h, int32_t n_sig, int64_t stride, const int64_t* lengths_host,
                                   int32_t fs, const float* est, const float* ref, int32_t kind, float* loss,
                                   float* counted, float* g, float* sums, void* workspace, size_t workspace_bytes,
                                   void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    StoiLayout Lo;
    int64_t max_len;
    // (the per-sample kernels take ceil(stride / 256) workgroups in grid.x, which must stay below 2^31)
    if (stride > ((int64_t)1 << 38))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "stoi_loss: bad argument (stride = %lld above 2^38)", (long long)stride);
    const int32_t rc = stoi_check(h, "stoi_loss", n_sig, stride, lengths_host, fs, est, ref,
                                  loss && counted && g && sums, true, Lo, max_len);
    if (rc != DRNMF_OK) return rc;
    if (kind != DRNMF_STOI_LOSS_STOI)
        DRNMF_FAIL(h, DRNMF_ERR_UNSUPPORTED, "stoi_loss: kind = %d unsupported (DRNMF_STOI_LOSS_STOI only)", kind);
    const StoiLossLayout G = stoi_loss_layout(Lo, n_sig);
    if (!workspace || workspace_bytes < G.total)
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "stoi_loss: workspace too small (%zu < %zu bytes)",
                   workspace ? workspace_bytes : (size_t)0, G.total);
    if (((uintptr_t)workspace & 255) != 0)
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "stoi_loss: workspace is not 256-byte aligned");
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "stoi_loss: the handle is bound to no device");
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    const StoiFront fr = stoi_front(Lo, n_sig, stride, lengths_host, max_len, est, ref, nullptr, nullptr, nullptr, ws,
                                    stream);
    float* stoi = (float*)(ws + G.off_stoi);
    stoi_back(Lo, n_sig, fr, stoi, ws, stream);
    hipLaunchKernelGGL(stoi_loss_rows_kernel, dim3(1), dim3(256), 0, stream, (const float*)stoi, n_sig, loss,
                       counted, sums);
    double* sb = (double*)(ws + G.off_sb);
    double* gy = (double*)(ws + G.off_gy);
    double* frg = (double*)(ws + G.off_fr);
    const int64_t* lens = (const int64_t*)(ws + Lo.off_len);
    const int* kidx = (const int*)(ws + Lo.off_kidx);
    const int V = Lo.V > 0 ? Lo.V : 1;
    const unsigned ns = (unsigned)n_sig;
    hipLaunchKernelGGL(stoi_loss_seg_kernel, dim3((unsigned)((Lo.S * ST_J + 255) / 256), ns), dim3(256), 0, stream,
                       fr.envx, fr.envy, fr.nk, Lo.F, Lo.S, sb);
    hipLaunchKernelGGL(stoi_loss_env_kernel, dim3((unsigned)((Lo.F * ST_J + 255) / 256), ns), dim3(256), 0, stream,
                       fr.envx, fr.envy, fr.nk, Lo.F, Lo.S, (const double*)sb, gy);
    const dim3 band_grid((unsigned)((Lo.F + 3) / 4), ns);
    const dim3 out_grid((unsigned)((stride + 255) / 256), ns);
    if (Lo.rs) {
        double* gr = (double*)(ws + G.off_gr);
        const int64_t rmax = resampled_len_h(max_len, Lo.p, Lo.q);
        hipLaunchKernelGGL(stoi_loss_band_kernel<double>, band_grid, dim3(256), 0, stream,
                           (const double*)(ws + Lo.off_yr), Lo.rstride, kidx, fr.nk, V, Lo.F, (const double*)gy, frg);
        hipLaunchKernelGGL(stoi_loss_gather_kernel<double>, dim3((unsigned)((rmax + 255) / 256 > 0 ? (rmax + 255) / 256 : 1), ns),
                           dim3(256), 0, stream, (const double*)frg, kidx, fr.nk, lens, (const float*)stoi, Lo.p, Lo.q,
                           V, Lo.F, rmax, gr, Lo.rstride);
        hipLaunchKernelGGL(stoi_loss_resample_kernel, out_grid, dim3(256), (size_t)Lo.L * sizeof(double), stream,
                           (const double*)gr, Lo.rstride, lens, (const float*)stoi, Lo.p, Lo.q, Lo.L,
                           (const double*)(ws + Lo.off_taps), g, stride);
    } else {
        hipLaunchKernelGGL(stoi_loss_band_kernel<float>, band_grid, dim3(256), 0, stream, est, stride, kidx, fr.nk, V,
                           Lo.F, (const double*)gy, frg);
        hipLaunchKernelGGL(stoi_loss_gather_kernel<float>, out_grid, dim3(256), 0, stream, (const double*)frg, kidx,
                           fr.nk, lens, (const float*)stoi, Lo.p, Lo.q, V, Lo.F, stride, g, stride);
    }
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}
