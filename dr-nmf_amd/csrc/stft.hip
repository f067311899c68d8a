// STFT-magnitude front end on gfx950.
//
// Reference: wavread's /32768 scaling (util.py:29-35), stft_mc (util.py:171-201: pad the signal
// to a multiple of hop, N zeros on both sides, librosa stft(center=False)), the sqrt-Hann window
// (audio_dataset.py:194) and the 'mag' transform sqrt(re^2 + im^2) (audio_dataset.py:22-23).
// librosa 0.5.1 conjugates the spectrum; the magnitude this path produces is unaffected.
//
// One workgroup per (signal, frame): window + zero-padded framing on load, an in-LDS radix-2
// FFT (bit-reversed load, two butterfly stages per pass; window and twiddles from per-size tables), and the
// magnitude of bins 0..N/2 written as one coalesced row.  fp32 arithmetic as in the reference (scipy
// fftpack on float32 input).  Measured (bench.py extra.stft_front_end, 64 x 10 s at 16 kHz, N = 1024,
// hop = 256): 217 us = 186 M frames/s, 475 GB/s in + out -- 5.9 % of the HBM rate: the FFT passes are
// LDS-latency / barrier bound (two radix-2 stages per pass: 293 -> 217 us together with the tables),
// not memory bound; the front end is ~600x faster than the recurrent cell consumes frames.
#include "common.h"
#include "../../include/drnmf_enhance.h"
#include "../../include/drnmf_dataset.h"
#include "../../include/drnmf_target.h"
#include "../../include/drnmf_stream.h"
#include "../../include/drnmf_waveloss.h"

namespace {

// in-place radix-2 DIT FFT of N complex points in LDS (input already bit-reversed); tw[k] =
// e^{-2 pi i k / N}, k < N/2
__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
    return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

__device__ __forceinline__ void fft_lds(float2* buf, const float2* tw, int N, int logN, int tid) {
    int s = 1;
    if (logN & 1) {                      // odd log2 N: one radix-2 stage first
        for (int b = tid; b < N / 2; b += 256) {
            const float2 u = buf[2 * b], v = buf[2 * b + 1];      // twiddle 1
            buf[2 * b] = make_float2(u.x + v.x, u.y + v.y);
            buf[2 * b + 1] = make_float2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
        s = 2;
    }
    // two radix-2 stages (s, s+1) per pass, the intermediate values in registers: half the LDS
    // round trips and barriers of the stage-by-stage loop (the kernel is bound by those, not by
    // memory); the butterflies and their order are exactly the radix-2 ones
    for (; s < logN; s += 2) {
        const int half = 1 << (s - 1);
        const int ts1 = N >> s, ts2 = N >> (s + 1);
        for (int b = tid; b < N / 4; b += 256) {
            const int pos = b & (half - 1);
            const int base = ((b >> (s - 1)) << (s + 1)) + pos;
            const float2 w1 = tw[pos * ts1], w2 = tw[pos * ts2], w3 = tw[(pos + half) * ts2];
            const float2 p0 = buf[base], p1 = buf[base + half], p2 = buf[base + 2 * half],
                         p3 = buf[base + 3 * half];
            const float2 t1 = cmul(p1, w1), t3 = cmul(p3, w1);
            const float2 a0 = make_float2(p0.x + t1.x, p0.y + t1.y);
            const float2 a1 = make_float2(p0.x - t1.x, p0.y - t1.y);
            const float2 a2 = make_float2(p2.x + t3.x, p2.y + t3.y);
            const float2 a3 = make_float2(p2.x - t3.x, p2.y - t3.y);
            const float2 u2 = cmul(a2, w2), u3 = cmul(a3, w3);
            buf[base] = make_float2(a0.x + u2.x, a0.y + u2.y);
            buf[base + 2 * half] = make_float2(a0.x - u2.x, a0.y - u2.y);
            buf[base + half] = make_float2(a1.x + u3.x, a1.y + u3.y);
            buf[base + 3 * half] = make_float2(a1.x - u3.x, a1.y - u3.y);
        }
        __syncthreads();
    }
}

// Window and twiddle tables per FFT size (64 .. 4096 = 2^6 .. 2^12), in static device memory and
// refilled by every call (a handful of threads; concurrent callers write identical values): the
// per-frame workgroups read them from L2 instead of evaluating 2N transcendental functions each
// (the window needs a double-precision cospi to reproduce float32(hann) exactly).
constexpr int TAB_LOG_MIN = 6, TAB_LOG_MAX = 12, TAB_N_MAX = 1 << TAB_LOG_MAX;
__device__ float g_window[TAB_LOG_MAX - TAB_LOG_MIN + 1][TAB_N_MAX];
__device__ float2 g_twiddle[TAB_LOG_MAX - TAB_LOG_MIN + 1][TAB_N_MAX / 2];

__device__ __forceinline__ float sqrt_hann(int i, int N) {
    // sqrt(hann(N, sym=False)) with the Hann value rounded to float32 first (audio_dataset.py:194)
    const float hann = (float)(0.5 - 0.5 * cospi(2.0 * (double)i / (double)N));
    return sqrtf(hann);
}

__global__ void __launch_bounds__(256) fft_tables_kernel(int N, int logN) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) g_window[logN - TAB_LOG_MIN][i] = sqrt_hann(i, N);
    if (i < N / 2) {
        float sn, cs;
        sincospif(-2.0f * (float)i / (float)N, &sn, &cs);
        g_twiddle[logN - TAB_LOG_MIN][i] = make_float2(cs, sn);
    }
}

// the feature transform of a magnitude (audio_dataset.py:22-28): 0 'mag', 1 'logmag' = log(1 + m) in the
// reference's own expression (not log1pf).  Every caller passes a constant 0 or a kernel argument.
__device__ __forceinline__ float mag_transform(float m, int transform) {
    return transform ? logf(1.0f + m) : m;
}

// The training target of include/drnmf_target.h from one bin of the clean (s) and of the noisy (x) member:
// p = (re_s re_x + im_s im_x) / m_x = |S| cos(theta_S - theta_X), 0 where m_x == 0; 'tpsa' clips it to [0, m_x].
// Two products, one sum and one true division, each rounded once: no contraction, so the value does not depend
// on which kernel the expression is inlined into.
__device__ __forceinline__ float psa_target(float re_s, float im_s, float re_x, float im_x, float m_x, int target) {
#pragma clang fp contract(off)
    float p = 0.f;
    if (m_x > 0.f) {
        const float a = re_s * re_x, b = im_s * im_x;
        p = (a + b) / m_x;
    }
    return target == DRNMF_TARGET_TPSA ? fminf(fmaxf(p, 0.f), m_x) : p;
}

// What a target kernel (stft_pair_target_*) carries through the two runs of its frame body.  A lane emits the
// SAME bins of both members (slot s of a lane is one bin), so the noisy member's re, im and magnitude wait in
// that lane's registers while the clean member is transformed: nothing is exchanged between lanes, nothing goes
// through LDS or global memory.  side 0 (noisy): the body's magnitude is stored as it is and the bin is kept;
// side 1 (clean): the target is stored in its place.  NoTarget: every other kernel, whose bodies are unchanged.
template <int SLOTS>
struct PairTarget {
    static constexpr bool on = true;
    static constexpr int slots = SLOTS;
    int side, target;
    float re[SLOTS], im[SLOTS], m[SLOTS];
    __device__ __forceinline__ float bin(int s, float re_k, float im_k, float m_k, float out_k) {
        if (side == 0) {
            re[s] = re_k, im[s] = im_k, m[s] = m_k;
            return out_k;
        }
        return psa_target(re_k, im_k, re[s], im[s], m[s], target);
    }
};
struct NoTarget {
    static constexpr bool on = false;
};

// one frame of one signal by the whole workgroup: row0 = element offset of the signal's first sample in pcm,
// nsampl its length, o = element offset of the frame's output row (shared by the batched, the ragged and the
// paired kernel).  Each of mag / re / im is written only if its pointer is not NULL.  stage_tw = false: tw
// already holds this size's twiddles (the second member of a pair); the caller has put a barrier behind the
// previous frame's reads of buf.  tg: see PairTarget (thread tid emits bin tid + 256 s in slot s).
template <class TG = NoTarget>
__device__ __forceinline__ void stft_frame(const void* __restrict__ pcm, int is_int16, size_t row0,
                                           int64_t nsampl, int N, int logN, int hop, int frame, size_t o,
                                           float* __restrict__ mag, float* __restrict__ re,
                                           float* __restrict__ im, float2* buf, float2* tw, int tid,
                                           int transform = 0, bool stage_tw = true, TG* tg = nullptr) {
    const int64_t base = (int64_t)frame * hop - N;   // first sample of the frame (N leading zeros)

    const float* __restrict__ win = g_window[logN - TAB_LOG_MIN];
    if (stage_tw)
        for (int k = tid; k < N / 2; k += 256) tw[k] = g_twiddle[logN - TAB_LOG_MIN][k];
    for (int i = tid; i < N; i += 256) {
        const int64_t idx = base + i;
        float v = 0.f;
        if (idx >= 0 && idx < nsampl) {
            v = is_int16 ? (float)((const short*)pcm)[row0 + idx] / 32768.0f
                         : ((const float*)pcm)[row0 + idx];
        }
        v *= win[i];
        const unsigned rev = __brev((unsigned)i) >> (32 - logN);
        buf[rev] = make_float2(v, 0.f);
    }
    __syncthreads();
    fft_lds(buf, tw, N, logN, tid);
    if constexpr (TG::on) {
        // the loop below with its trips counted at compile time, so that the slots are registers
#pragma unroll
        for (int s = 0; s < TG::slots; ++s) {
            const int k = tid + 256 * s;
            if (k <= N / 2) {
                const float2 z = buf[k];
                const float m = sqrtf(z.x * z.x + z.y * z.y);
                if (mag) mag[o + k] = tg->bin(s, z.x, -z.y, m, mag_transform(m, transform));
                if (re) re[o + k] = z.x;
                if (im) im[o + k] = -z.y;
            }
        }
        return;
    }
    for (int k = tid; k <= N / 2; k += 256) {
        const float2 z = buf[k];
        if (mag) mag[o + k] = mag_transform(sqrtf(z.x * z.x + z.y * z.y), transform);
        if (re) re[o + k] = z.x;
        if (im) im[o + k] = -z.y;    // librosa 0.5.1 conjugates the spectrum (util.py:195 via stft)
    }
}

__global__ void __launch_bounds__(256)
stft_kernel(const void* __restrict__ pcm, int is_int16, int64_t nsampl, int N, int logN, int hop,
            int nf, float* __restrict__ mag, float* __restrict__ re, float* __restrict__ im) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float2* buf = (float2*)smem;            // N complex points
    float2* tw = buf + N;                   // N/2 twiddles e^{-2 pi i k / N}
    const int frame = blockIdx.x, sig = blockIdx.y;
    stft_frame(pcm, is_int16, (size_t)sig * nsampl, nsampl, N, logN, hop, frame,
               ((size_t)sig * nf + frame) * (N / 2 + 1), mag, re, im, buf, tw, threadIdx.x);
}


// ---------------------------------------------------------------------------------------------
// Fast path for the sizes the reference uses (N = 512 shipped, N = 1024 in BASELINE): the input is
// real, so a frame is ONE complex FFT of M = N/2 points, z[n] = x[2n] + i x[2n+1], followed by the
// split X[k] = (Z[k] + conj Z[M-k]) / 2 - i e^{-2 pi i k / N} (Z[k] - conj Z[M-k]) / 2.  The M-point
// FFT is a Stockham autosort of radix-R passes (R = 8 for M = 512, R = 4 for M = 256) with the R
// points of a butterfly in registers: M / R = 64 butterflies = ONE WAVE per frame, so the passes
// exchange through a wave-private LDS slice with no workgroup barrier; a 256-thread workgroup
// carries 4 frames.  Against the radix-2 kernel above (one workgroup per frame, a complex FFT twice
// the size, a barrier every two stages) it moves the front end from LDS latency towards HBM.
template <int R>
__device__ __forceinline__ void dft_r(float2 (&v)[R]);

template <>
__device__ __forceinline__ void dft_r<4>(float2 (&v)[4]) {
    const float2 a = make_float2(v[0].x + v[2].x, v[0].y + v[2].y);
    const float2 b = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
    const float2 c = make_float2(v[1].x + v[3].x, v[1].y + v[3].y);
    const float2 d = make_float2(v[1].x - v[3].x, v[1].y - v[3].y);
    v[0] = make_float2(a.x + c.x, a.y + c.y);
    v[2] = make_float2(a.x - c.x, a.y - c.y);
    v[1] = make_float2(b.x + d.y, b.y - d.x);      // b - i d
    v[3] = make_float2(b.x - d.y, b.y + d.x);      // b + i d
}

template <>
__device__ __forceinline__ void dft_r<8>(float2 (&v)[8]) {
    float2 e[4] = {v[0], v[2], v[4], v[6]}, o[4] = {v[1], v[3], v[5], v[7]};
    dft_r<4>(e);
    dft_r<4>(o);
    const float h = 0.70710678118654752440f;
    // o[r] *= e^{-2 pi i r / 8}
    o[1] = make_float2(h * (o[1].x + o[1].y), h * (o[1].y - o[1].x));
    o[2] = make_float2(o[2].y, -o[2].x);
    o[3] = make_float2(h * (o[3].y - o[3].x), -h * (o[3].x + o[3].y));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        v[r] = make_float2(e[r].x + o[r].x, e[r].y + o[r].y);
        v[r + 4] = make_float2(e[r].x - o[r].x, e[r].y - o[r].y);
    }
}

template <int R, int P>
struct RealFft {                          // M = R^P complex points, N = 2M real samples
    static constexpr int M = (R == 8 ? (P == 3 ? 512 : 64) : (P == 4 ? 256 : 64)), N = 2 * M;
    // per wave: ONE buffer, rewritten in place by every pass -- a wave executes its LDS reads of a
    // pass (all 64 lanes, into registers) before that pass's writes are issued, and LDS serves one
    // wave's requests in order, so the Stockham reorder needs no second buffer (the ping-pong pair
    // it replaced held the kernel to 3 workgroups per CU; 7 now).  Index i lives at i + i/8: the
    // scatter of the early passes (stride R, then R*R) would otherwise put 8-16 lanes on one bank
    static constexpr int MP = M + M / 8;
    static __device__ __forceinline__ int pad(int i) { return i + (i >> 3); }
};

// The P radix-R Stockham passes of one wave (lane j): v[r] = z[j + r M/R] on entry, Z[k] = sum_n z[n]
// e^{-2 pi i k n / M} at cur[pad(k)] on return; tw = e^{-2 pi i k / N}, k < N/2, in LDS.
template <int R, int P>
__device__ __forceinline__ void stockham_passes(float2 (&v)[R], float2* cur, const float2* tw, int j) {
    constexpr int M = RealFft<R, P>::M, N = 2 * M;
    auto pad = [](int i) { return RealFft<R, P>::pad(i); };
    auto twid = [&](int idx) {                // e^{-2 pi i idx / N}, 0 <= idx < N
        const float2 t = tw[idx & (N / 2 - 1)];
        return idx >= N / 2 ? make_float2(-t.x, -t.y) : t;
    };
    float2* nxt = cur;
    int Ns = 1;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        if (p > 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) v[r] = cur[pad(j + r * (M / R))];
        }
        const int k = j & (Ns - 1);
        if (p > 0) {                          // twiddles e^{-2 pi i k r / (Ns R)} (pass 0: k = 0)
            const int step = k * (N / (Ns * R));
#pragma unroll
            for (int r = 1; r < R; ++r) v[r] = cmul(v[r], twid(step * r));
        }
        dft_r<R>(v);
        const int j0 = (j - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) nxt[pad(j0 + r * Ns)] = v[r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        Ns *= R;
    }
}

// one frame of one signal by ONE WAVE (lane j): row0 = element offset of the signal's first sample in pcm,
// nsampl its length, o = element offset of the frame's output row (shared by the batched, the ragged and the
// paired kernel).  Each of mag / re / im is written only if its pointer is not NULL.  tg: see PairTarget (lane j
// emits bin j + 64 s in slot s < M/64, and lane 0 bin M in slot M/64).
template <int R, int P, class TG = NoTarget>
__device__ __forceinline__ void stft_real_frame(const void* __restrict__ pcm, int is_int16, size_t row0,
                                                int64_t nsampl, int logN, int hop, int frame, size_t o,
                                                float* __restrict__ mag, float* __restrict__ re,
                                                float* __restrict__ im, const float2* tw, float2* cur, int j,
                                                int transform = 0, TG* tg = nullptr) {
    constexpr int M = RealFft<R, P>::M, N = 2 * M;
    auto pad = [](int i) { return RealFft<R, P>::pad(i); };
    const float* __restrict__ win = g_window[logN - TAB_LOG_MIN];
    // pass 0 input straight from the signal: z[n] = (x[2n] w[2n], x[2n+1] w[2n+1]), n = j + r M/R
    const int64_t base = (int64_t)frame * hop - N;       // first sample of the frame (N leading zeros)
    float2 v[R];
    // interior frames (all but the first N/hop and the last few): no bounds tests, one 8-byte load
    // per sample pair -- this kernel is VALU-issue bound (~1000 instructions per lane and frame),
    // the 16 64-bit range tests were a tenth of them
    const size_t e0 = row0 + (size_t)(base > 0 ? base : 0);   // first element
    const bool interior = base >= 0 && base + N <= nsampl &&
                          ((((uintptr_t)pcm >> (is_int16 ? 1 : 2)) + e0) & 1) == 0;
    if (interior && is_int16) {
        const short* p = (const short*)pcm + e0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int n = j + r * (M / R);
            const short2 x2 = *(const short2*)(p + 2 * n);
            const float2 w2 = *(const float2*)(win + 2 * n);
            v[r] = make_float2((float)x2.x / 32768.0f * w2.x, (float)x2.y / 32768.0f * w2.y);
        }
    } else if (interior) {
        const float* p = (const float*)pcm + e0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int n = j + r * (M / R);
            const float2 x2 = *(const float2*)(p + 2 * n);
            const float2 w2 = *(const float2*)(win + 2 * n);
            v[r] = make_float2(x2.x * w2.x, x2.y * w2.y);
        }
    } else
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int n = j + r * (M / R);
        const int64_t i0 = base + 2 * n;
        float x0 = 0.f, x1 = 0.f;
        if (is_int16) {
            const short* p = (const short*)pcm + row0;
            if (i0 >= 0 && i0 < nsampl) x0 = (float)p[i0] / 32768.0f;
            if (i0 + 1 >= 0 && i0 + 1 < nsampl) x1 = (float)p[i0 + 1] / 32768.0f;
        } else {
            const float* p = (const float*)pcm + row0;
            if (i0 >= 0 && i0 < nsampl) x0 = p[i0];
            if (i0 + 1 >= 0 && i0 + 1 < nsampl) x1 = p[i0 + 1];
        }
        const float2 w2 = *(const float2*)(win + 2 * n);
        v[r] = make_float2(x0 * w2.x, x1 * w2.y);
    }
    stockham_passes<R, P>(v, cur, tw, j);
    // split + output: k = j + 64 i, i < M/64, and k = M
    auto emit = [&](int k, int slot) {
        const float2 zk = cur[pad(k & (M - 1))];
        const float2 zc = cur[pad((M - k) & (M - 1))];     // Z[M-k] (Z[M] = Z[0])
        const float2 a = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y - zc.y));   // (Z_k + conj Z_{M-k}) / 2
        const float2 b = make_float2(0.5f * (zk.x - zc.x), 0.5f * (zk.y + zc.y));   // (Z_k - conj Z_{M-k}) / 2
        const float2 w = k == M ? make_float2(-1.f, 0.f) : tw[k];
        const float2 wb = cmul(b, w);                       // X = a - i w b
        const float xr = a.x + wb.y, xi = a.y - wb.x;
        if constexpr (TG::on) {
            const float m = sqrtf(xr * xr + xi * xi);
            if (mag) mag[o + k] = tg->bin(slot, xr, -xi, m, mag_transform(m, transform));
        } else {
            if (mag) mag[o + k] = mag_transform(sqrtf(xr * xr + xi * xi), transform);
        }
        if (re) re[o + k] = xr;
        if (im) im[o + k] = -xi;      // librosa 0.5.1 conjugates the spectrum (util.py:195 via stft)
    };
#pragma unroll
    for (int i = 0; i < M / 64; ++i) emit(j + 64 * i, i);
    if (j == 0) emit(M, M / 64);
}


template <int R, int P>
__global__ void __launch_bounds__(256)
stft_real_kernel(const void* __restrict__ pcm, int is_int16, int64_t nsampl, int logN, int hop,
                 int nf, float* __restrict__ mag, float* __restrict__ re, float* __restrict__ im) {
    constexpr int N = RealFft<R, P>::N;
    __shared__ float2 tw[N / 2];              // e^{-2 pi i k / N}, k < N/2
    __shared__ float2 bufs[4][RealFft<R, P>::MP];
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    const int frame = blockIdx.x * 4 + wv, sig = blockIdx.y;
    for (int k = tid; k < N / 2; k += 256) tw[k] = g_twiddle[logN - TAB_LOG_MIN][k];
    __syncthreads();
    if (frame >= nf) return;                  // (whole waves: no barrier below)
    stft_real_frame<R, P>(pcm, is_int16, (size_t)sig * nsampl, nsampl, logN, hop, frame,
                          ((size_t)sig * nf + frame) * (N / 2 + 1), mag, re, im, tw, bufs[wv], j);
}

// ---------------------------------------------------------------------------------------------
// The host half.  Every entry that launches an FFT kernel takes its size from three shared pieces:
// check_fft_size (one predicate, one message), fft_call (log2 N, the generic kernels' dynamic LDS, the tables
// on the caller's stream) and with_fft_size (which kernel of a family runs a size).  What an entry keeps for
// itself is the ORDER of its checks and the CODE of its size check -- callers see which error wins when two
// apply, and tests/test_stft_args_host.py pins it:
//   drnmf_stft_mag                  shape, N (UNSUPPORTED), NULL
//   drnmf_stft                      "bad argument" (shape or NULL), N (UNSUPPORTED); is_int16 is not checked
//   drnmf_istft_masked              "bad argument", N (UNSUPPORTED), workspace
//   drnmf_stft_ragged               shape, N, NULL
//   drnmf_istft_ragged              shape, N, NULL, ld_mask, workspace
//   drnmf_istft_ragged_vjp          shape, N, NULL, ld_dm
//   drnmf_stft_pair_chunks          n_seq / T, then check_stft_pair (shape, N, transform, frame overflow), NULL
//   drnmf_stft_pair_chunks_target   target, the chunks' checks, target needs TRANSFORM_MAG, unbound handle (the
//                                   only entry that tests h->device)
//   drnmf_stft_pair_frames          total_frames, check_stft_pair, NULL
//   drnmf_stream_reset              check_stream (B, N, hop, NULL state, state bytes)
//   drnmf_stream_forward            shape, NULL, check_stream
//   drnmf_stream_inverse            shape, NULL, check_stream, ld_mask
// N is INVALID_ARG where no code is named.  drnmf_stream_state_bytes answers 0 from the same predicate.
static_assert(TAB_LOG_MIN == 6 && TAB_LOG_MAX == 12, "check_fft_size's message says [64,4096]");

static bool fft_size_ok(int N) { return N >= (1 << TAB_LOG_MIN) && N <= TAB_N_MAX && (N & (N - 1)) == 0; }

static int32_t check_fft_size(drnmf_handle_t h, const char* who, int N, int32_t code) {
    if (!fft_size_ok(N)) DRNMF_FAIL(h, code, "%s: N=%d must be a power of two in [64,4096]", who, N);
    return DRNMF_OK;
}

// Which kernel of a family runs size N: f(FftSize<8, 3>) for N = 1024 and f(FftSize<4, 4>) for N = 512, the
// RealFft<R, P> kernels (one wave per frame, static LDS); f(AnySize) for every other size, the radix-2 kernels (one
// workgroup per frame, FftCall::lds of dynamic LDS).  A third fast size is a line here.
template <int R_, int P_>
struct FftSize {
    static constexpr int R = R_, P = P_;
    static constexpr bool fast = R_ != 0;
};
using AnySize = FftSize<0, 0>;

template <class Fn>
static void with_fft_size(int N, Fn&& f) {
    if (N == RealFft<8, 3>::N) f(FftSize<8, 3>{});
    else if (N == RealFft<4, 4>::N) f(FftSize<4, 4>{});
    else f(AnySize{});
}

static bool stft_fast(int N) {
    bool fast = false;
    with_fft_size(N, [&](auto s) { fast = decltype(s)::fast; });
    return fast;
}

// The window / twiddle tables of a size are filled once per handle (= per device); later calls on
// any stream only wait for the event recorded behind that fill.
static int32_t ensure_fft_tables(drnmf_handle_t h, int N, int logN, hipStream_t stream) {
    const int slot = logN - TAB_LOG_MIN;
    if (!h->fft_ready[slot]) {
        hipLaunchKernelGGL(fft_tables_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0,
                           stream, N, logN);
        DRNMF_HIP(h, hipGetLastError());
        DRNMF_HIP(h, hipEventCreateWithFlags(&h->fft_event[slot], hipEventDisableTiming));
        DRNMF_HIP(h, hipEventRecord(h->fft_event[slot], stream));
        h->fft_ready[slot] = true;
    } else {
        DRNMF_HIP(h, hipStreamWaitEvent(stream, h->fft_event[slot], 0));
    }
    return DRNMF_OK;
}

// What every launch of an FFT kernel needs of a checked size; filled by fft_call and by nothing else.
struct FftCall {
    int N, logN;
    size_t lds;                   // dynamic LDS of the AnySize kernels: N points and N/2 twiddles
    hipStream_t stream;
};

static int32_t fft_call(drnmf_handle_t h, int N, void* stream_, FftCall* c) {
    c->N = N;
    c->logN = 0;
    while ((1 << c->logN) < N) ++c->logN;
    c->lds = (size_t)(N + N / 2) * sizeof(float2);
    c->stream = (hipStream_t)stream_;
    return ensure_fft_tables(h, N, c->logN, c->stream);
}

// one workgroup per (signal, frame): masked spectrum -> Hermitian extension -> inverse FFT -> real
// part * window * 2/(N/hop)  (util.py:48-169 istft_noDiv with center=False).  o, om = element offsets of the
// frame's spectrum and mask rows, out = its N output samples (shared by the batched and the ragged kernel)
__device__ __forceinline__ void istft_frame(const float* __restrict__ re, const float* __restrict__ im,
                                            const float* __restrict__ mask, size_t o, size_t om, int N,
                                            int logN, int hop, float* __restrict__ out, float2* buf,
                                            float2* tw, int tid) {
    const float* __restrict__ win = g_window[logN - TAB_LOG_MIN];
    for (int k = tid; k < N / 2; k += 256) tw[k] = g_twiddle[logN - TAB_LOG_MIN][k];
    // ifft(z) = conj(fft(conj(z)))/N.  With S the stored (conjugated) spectrum the reference
    // builds z = [conj(S_0..S_{N/2}), S_{N/2-1}..S_1], so conj(z) = [S_k ; conj(S_{N-k})].
    for (int k = tid; k < N; k += 256) {
        const int kk = k <= N / 2 ? k : N - k;
        const float m = mask ? mask[om + kk] : 1.f;
        float2 z = make_float2(m * re[o + kk], m * im[o + kk]);
        if (k > N / 2) z.y = -z.y;
        const unsigned rev = __brev((unsigned)k) >> (32 - logN);
        buf[rev] = z;
    }
    __syncthreads();
    fft_lds(buf, tw, N, logN, tid);
    const float scale = (2.0f / ((float)N / (float)hop)) / (float)N;
    for (int i = tid; i < N; i += 256) out[i] = buf[i].x * scale * win[i];
}

__global__ void __launch_bounds__(256)
istft_frames_kernel(const float* __restrict__ re, const float* __restrict__ im,
                    const float* __restrict__ mask, int N, int logN, int hop, int nf,
                    float* __restrict__ frames) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float2* buf = (float2*)smem;
    float2* tw = buf + N;
    const int frame = blockIdx.x, sig = blockIdx.y;
    const size_t o = ((size_t)sig * nf + frame) * (N / 2 + 1);
    istft_frame(re, im, mask, o, o, N, logN, hop, frames + ((size_t)sig * nf + frame) * N, buf, tw,
                threadIdx.x);
}

// overlap-add by gathering (deterministic), with istft_mc's trimming of the N padding samples on
// both sides and the crop to nsampl (util.py:203-226)
__global__ void __launch_bounds__(256)
overlap_add_kernel(const float* __restrict__ frames, int N, int hop, int nf, int64_t nsampl,
                   float* __restrict__ y) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int sig = blockIdx.y;
    if (s >= nsampl) return;
    const int64_t p = s + N;                                  // index in the untrimmed signal
    const int64_t total = (int64_t)N + (int64_t)hop * (nf - 1);
    float acc = 0.f;
    if (p < total - N) {
        int64_t j0 = (p - N + hop) / hop;                     // ceil((p - N + 1) / hop)
        if (j0 < 0) j0 = 0;
        int64_t j1 = p / hop;
        if (j1 > nf - 1) j1 = nf - 1;
        for (int64_t j = j0; j <= j1; ++j)
            acc += frames[((size_t)sig * nf + j) * N + (p - j * hop)];
    }
    y[(size_t)sig * nsampl + s] = acc;
}

// SNR = 10 log10(sum ref^2 / sum (ref - est)^2)  (score_audio.m:209), one workgroup per signal
__global__ void __launch_bounds__(256)
snr_kernel(const float* __restrict__ est, const float* __restrict__ ref, int64_t nsampl,
           float* __restrict__ out_db) {
    __shared__ double s0[256], s1[256];
    const int sig = blockIdx.x;
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < nsampl; i += 256) {
        const double r = ref[(size_t)sig * nsampl + i], e = est[(size_t)sig * nsampl + i];
        a += r * r;
        b += (r - e) * (r - e);
    }
    s0[threadIdx.x] = a;
    s1[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s0[threadIdx.x] += s0[threadIdx.x + o];
            s1[threadIdx.x] += s1[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out_db[sig] = (float)(10.0 * log10(s0[0] / s1[0]));
}

// Frames of a signal of len samples: stft_mc pads it to a multiple of hop (util.py:183) and puts N zeros on both
// sides, and librosa frames that with center=False.  drnmf_stft_frames and drnmf_stream_counts on the host,
// ragged_row on the device; pair_row and stream_push keep the rule written out (see there).
__host__ __device__ inline int64_t stft_frame_count(int64_t len, int N, int hop) {
    const int64_t nfram = (len + hop - 1) / hop;
    return 1 + (nfram * hop + (int64_t)N) / hop;
}

// ---------------------------------------------------------------------------------------------
// Ragged batches (include/drnmf_enhance.h): the signals of a slab have their own lengths, read on the device;
// slab row k = signal sig_index[k].  What a row computes depends on its own signal only.
struct RaggedRow {
    int sig;              // -1: sig_index[k] outside [0, n_sig)
    int64_t len;          // lengths[sig] taken into [0, cap]
    int64_t nf;           // drnmf_stft_frames(len, N, hop)
};

__device__ __forceinline__ RaggedRow ragged_row(const int64_t* __restrict__ lengths,
                                                const int* __restrict__ sig_index, int n_sig, int k,
                                                int64_t cap, int N, int hop) {
    RaggedRow r;
    r.sig = sig_index[k];
    if (r.sig < 0 || r.sig >= n_sig) {
        r.sig = -1;
        r.len = 0;
        r.nf = 0;
        return r;
    }
    int64_t len = lengths[r.sig];
    len = len < 0 ? 0 : (len > cap ? cap : len);
    r.len = len;
    r.nf = stft_frame_count(len, N, hop);
    return r;
}

// samples a row's reconstruction has: istft_mc trims N on both sides of N + hop (nf - 1) (util.py:203-226)
__device__ __forceinline__ int64_t ragged_nout(const RaggedRow& r, int N, int hop, int crop,
                                               int64_t stride_y) {
    int64_t n = (int64_t)hop * (r.nf - 1) - N;
    if (n < 0) n = 0;
    if (crop && r.len < n) n = r.len;
    return n < stride_y ? n : stride_y;
}

template <int R, int P>
__global__ void __launch_bounds__(256)
stft_real_ragged_kernel(const void* __restrict__ pcm, int is_int16, int64_t stride,
                        const int64_t* __restrict__ lengths, const int* __restrict__ sig_index, int n_sig,
                        int T, int logN, int hop, float mask_value, float* __restrict__ x,
                        float* __restrict__ re, float* __restrict__ im) {
    constexpr int N = RealFft<R, P>::N, F = N / 2 + 1;
    __shared__ float2 tw[N / 2];
    __shared__ float2 bufs[4][RealFft<R, P>::MP];
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    const int frame = blockIdx.x * 4 + wv, k = blockIdx.y;
    for (int i = tid; i < N / 2; i += 256) tw[i] = g_twiddle[logN - TAB_LOG_MIN][i];
    __syncthreads();
    if (frame >= T) return;                   // (whole waves: no barrier below)
    const RaggedRow row = ragged_row(lengths, sig_index, n_sig, k, stride, N, hop);
    const size_t o = ((size_t)k * T + frame) * F;
    if (frame >= row.nf) {                    // padding frame: Masking's value in every bin
        for (int i = j; i < F; i += 64) x[o + i] = mask_value;
        return;
    }
    stft_real_frame<R, P>(pcm, is_int16, (size_t)row.sig * stride, row.len, logN, hop, frame, o, x, re, im,
                          tw, bufs[wv], j);
}

__global__ void __launch_bounds__(256)
stft_ragged_kernel(const void* __restrict__ pcm, int is_int16, int64_t stride,
                   const int64_t* __restrict__ lengths, const int* __restrict__ sig_index, int n_sig, int T,
                   int N, int logN, int hop, float mask_value, float* __restrict__ x,
                   float* __restrict__ re, float* __restrict__ im) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float2* buf = (float2*)smem;
    float2* tw = buf + N;
    const int frame = blockIdx.x, k = blockIdx.y, F = N / 2 + 1;
    const RaggedRow row = ragged_row(lengths, sig_index, n_sig, k, stride, N, hop);
    const size_t o = ((size_t)k * T + frame) * F;
    if (frame >= row.nf) {                    // (the whole workgroup: no barrier is skipped by a part of it)
        for (int i = threadIdx.x; i < F; i += 256) x[o + i] = mask_value;
        return;
    }
    stft_frame(pcm, is_int16, (size_t)row.sig * stride, row.len, N, logN, hop, frame, o, x, re, im, buf, tw,
               threadIdx.x);
}

// one masked frame back to N samples by ONE WAVE (lane j), the mirror of stft_real_frame (the derivation stands
// in front of istft_real_ragged_kernel): o, om = element offsets of the frame's spectrum and mask rows; on return
// x[n] * window[n] * scale sits at cur[pad(n >> 1)].x / .y (n even / odd).  Shared by the ragged and the
// streaming inverse.
template <int R, int P>
__device__ __forceinline__ void istft_real_frame(const float* re, const float* im, const float* mask, size_t o,
                                                 size_t om, const float2* tw, float2* cur, const float* win,
                                                 float scale, int j) {
    constexpr int M = RealFft<R, P>::M;
    auto pad = [](int i) { return RealFft<R, P>::pad(i); };
    float2 v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int ka = j + r * (M / R), kc = M - ka;       // 0 <= ka < M, 1 <= kc <= M
        const float ma = mask ? mask[om + ka] : 1.f, mc = mask ? mask[om + kc] : 1.f;
        float2 a = make_float2(ma * re[o + ka], ma * im[o + ka]);
        float2 c = make_float2(mc * re[o + kc], mc * im[o + kc]);
        if (ka == 0) {
            a.y = 0.f;
            c.y = 0.f;
        }
        const float2 A = make_float2(a.x + c.x, a.y - c.y);   // W_k + conj W_{M-k}
        const float2 B = make_float2(a.x - c.x, a.y + c.y);   // W_k - conj W_{M-k}
        const float2 wB = cmul(B, tw[ka]);
        v[r] = make_float2(A.x - wB.y, A.y + wB.x);           // A + i w B
    }
    stockham_passes<R, P>(v, cur, tw, j);
#pragma unroll
    for (int i = 0; i < M / 64; ++i) {
        const int n = j + 64 * i;
        const float2 z = cur[pad(n)];
        const float2 w2 = *(const float2*)(win + 2 * n);
        cur[pad(n)] = make_float2(z.x * scale * w2.x, z.y * scale * w2.y);
    }
}

// Masked inverse for N = 512 / 1024, the mirror of stft_real_kernel.  The frame is real, so its N samples are
// ONE complex transform of M = N/2 points: with W_k = mask_k S_k (Hermitian, the imaginary parts of W_0 and
// W_M dropped as the real part of the full transform drops them) and x[n] = sum_{k<N} W_k e^{-2 pi i k n / N},
//   z[n] = x[2n] + i x[2n+1] = sum_{k<M} Z_k e^{-2 pi i k n / M},
//   Z_k = (W_k + conj W_{M-k}) + i e^{-2 pi i k / N} (W_k - conj W_{M-k}),
// the inverse of the forward kernel's split.  One wave per frame runs the same Stockham passes and leaves
// x * window * 2 / (N / hop) / N in its LDS slice.
//
// A workgroup owns a run of `run` = C hop consecutive output samples of one signal (<= 2048: 8 per thread, in
// registers) and computes EVERY frame that overlaps the run, four at a time in ascending order; after each
// group of four, thread i adds the frames covering its samples, again ascending.  A sample is therefore the
// sum of its frames in ascending frame order starting from 0, whatever the run, slab or batch: bitwise
// reproducible, no atomics, no frames workspace, every sample of y written once (zeros behind the row's own
// length included).  The N/hop - 1 frames a run shares with each neighbour are recomputed, not exchanged.
template <int R, int P>
__global__ void __launch_bounds__(256)
istft_real_ragged_kernel(const float* __restrict__ re, const float* __restrict__ im,
                         const float* __restrict__ mask, int64_t ld_mask,
                         const int64_t* __restrict__ lengths, const int* __restrict__ sig_index, int n_sig,
                         int T, int logN, int hop, int run, int crop, float* __restrict__ y,
                         int64_t stride_y) {
    constexpr int M = RealFft<R, P>::M, N = 2 * M, F = M + 1, MP = RealFft<R, P>::MP;
    constexpr int SPT = 8;                    // samples per thread: run <= 256 SPT
    __shared__ float2 tw[N / 2];
    __shared__ float2 bufs[4][MP];
    auto pad = [](int i) { return RealFft<R, P>::pad(i); };
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    const int k = blockIdx.y;
    const RaggedRow row = ragged_row(lengths, sig_index, n_sig, k, (int64_t)1 << 40, N, hop);
    if (row.sig < 0) return;                  // (uniform over the workgroup, as every exit below)
    const int64_t nout = ragged_nout(row, N, hop, crop, stride_y);
    const int64_t s0 = (int64_t)blockIdx.x * run;
    float* __restrict__ yrow = y + (size_t)row.sig * stride_y;
    if (s0 >= nout) {                         // behind the row's samples: zeros
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            const int i = tid + 256 * q;
            if (i < run && s0 + i < stride_y) yrow[s0 + i] = 0.f;
        }
        return;
    }
    for (int i = tid; i < N / 2; i += 256) tw[i] = g_twiddle[logN - TAB_LOG_MIN][i];
    __syncthreads();
    const float* __restrict__ win = g_window[logN - TAB_LOG_MIN];
    const float scale = (2.0f / ((float)N / (float)hop)) / (float)N;
    // sample s is position p = s + N of the untrimmed signal; frame f covers [f hop, f hop + N)
    const int64_t s1 = s0 + run < nout ? s0 + run : nout;          // samples [s0, s1) are summed
    const int64_t nfe = row.nf < T ? row.nf : T;                   // frames at or behind T are dropped
    const int64_t f_lo = s0 / hop + 1;                             // first f with f hop + N - 1 >= s0 + N
    int64_t f_hi = (s1 - 1 + N) / hop;                             // last f with f hop <= s1 - 1 + N
    if (f_hi > nfe - 1) f_hi = nfe - 1;
    float acc[SPT];
#pragma unroll
    for (int q = 0; q < SPT; ++q) acc[q] = 0.f;
    float2* cur = bufs[wv];
    for (int64_t fb = f_lo; fb <= f_hi; fb += 4) {
        const int64_t f = fb + wv;
        if (f <= f_hi) {
            const size_t o = ((size_t)k * T + (size_t)f) * F;
            const size_t om = ((size_t)k * T + (size_t)f) * (size_t)ld_mask;
            istft_real_frame<R, P>(re, im, mask, o, om, tw, cur, win, scale, j);
        }
        __syncthreads();
        // sample i of the run sits at n = s0 + i + N - f hop of frame f (|s0 - f hop| < run + N + hop: int)
        const int nb = (int)(s0 + N - fb * hop), wmax = (int)(f_hi - fb);
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            const int i = tid + 256 * q;
            if (i < run) {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const int n = nb + i - w * hop;
                    if (w <= wmax && n >= 0 && n < N) {
                        const float2 z = bufs[w][pad(n >> 1)];
                        acc[q] += (n & 1) ? z.y : z.x;
                    }
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
        const int i = tid + 256 * q;
        const int64_t s = s0 + i;
        if (i < run && s < stride_y) yrow[s] = s < nout ? acc[q] : 0.f;
    }
}

// other sizes: the two-stage scheme of drnmf_istft_masked on a [b][T][N] frames buffer
__global__ void __launch_bounds__(256)
istft_frames_ragged_kernel(const float* __restrict__ re, const float* __restrict__ im,
                           const float* __restrict__ mask, int64_t ld_mask,
                           const int64_t* __restrict__ lengths, const int* __restrict__ sig_index, int n_sig,
                           int T, int N, int logN, int hop, float* __restrict__ frames) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float2* buf = (float2*)smem;
    float2* tw = buf + N;
    const int frame = blockIdx.x, k = blockIdx.y;
    const RaggedRow row = ragged_row(lengths, sig_index, n_sig, k, (int64_t)1 << 40, N, hop);
    if (frame >= row.nf) return;              // (the whole workgroup)
    const size_t fr = (size_t)k * T + frame;
    istft_frame(re, im, mask, fr * (N / 2 + 1), fr * (size_t)ld_mask, N, logN, hop, frames + fr * N, buf, tw,
                threadIdx.x);
}

__global__ void __launch_bounds__(256)
overlap_add_ragged_kernel(const float* __restrict__ frames, const int64_t* __restrict__ lengths,
                          const int* __restrict__ sig_index, int n_sig, int T, int N, int hop, int crop,
                          float* __restrict__ y, int64_t stride_y) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    const RaggedRow row = ragged_row(lengths, sig_index, n_sig, k, (int64_t)1 << 40, N, hop);
    if (row.sig < 0 || s >= stride_y) return;
    const int64_t nout = ragged_nout(row, N, hop, crop, stride_y);
    const int64_t nfe = row.nf < T ? row.nf : T;
    float acc = 0.f;
    if (s < nout) {
        const int64_t p = s + N;                                  // index in the untrimmed signal
        int64_t j0 = (p - N + hop) / hop;                         // ceil((p - N + 1) / hop)
        int64_t j1 = p / hop;
        if (j1 > nfe - 1) j1 = nfe - 1;
        for (int64_t j = j0; j <= j1; ++j) acc += frames[((size_t)k * T + j) * N + (p - j * hop)];
    }
    y[(size_t)row.sig * stride_y + s] = acc;
}

// ---------------------------------------------------------------------------------------------
// Paired training tensors (include/drnmf_dataset.h): the noisy and the clean magnitude of a frame by the SAME
// workgroup, straight into fit()'s layout (chunks: [n_seq][T][F] padded with the mask value, plus the 0/1
// weights) or into packed rows (frames: row row0[s] + t).  The frame bodies are the ones above, called with
// re = im = NULL, so a magnitude is bitwise what drnmf_stft / drnmf_stft_ragged write for that signal and frame.
// The clean signal decides the frame count (fidx = y_fidx, audio_dataset.py:232-264); the noisy one is framed
// with its OWN length, as clipping its full STFT does (clip_x_to_y).
struct PairArgs {
    const void* pcm_x;            // [n_sig][stride_x] noisy
    const void* pcm_y;            // [n_sig][stride_y] clean
    const int64_t* len_x;
    const int64_t* len_y;
    int64_t stride_x, stride_y;
    const int* table;             // chunks: [n_rows][2] (signal, first frame)
    const int64_t* row0;          // frames: [n_sig] first output row of a signal
    int64_t total_frames;         // frames: rows of x / y
    float* x;
    float* y;
    float* w;                     // chunks: [n_rows][T]
    // always NULL: no spectrum is written.  They are ARGUMENTS, as in every other kernel that holds the frame
    // bodies, and not the constant: with the stores compiled out the bodies' values have other use counts, the
    // compiler contracts other multiply-adds, and the magnitude differs from drnmf_stft's in the last bit
    float* re;
    float* im;
    int n_sig, T, hop, logN, is_int16, transform;
    float mask_value;
    int row_base, tile_base;      // this launch's offset into the rows (grid.y) and the frame tiles (grid.x)
};

struct PairRow {                  // what a workgroup knows about its row (uniform over the workgroup)
    int sig;                      // -1: nothing of this row is a frame
    int64_t f0, nf, len_x, len_y, orow;   // first frame, the clean side's frame count, output row of t = 0
};

template <bool PACKED>
__device__ __forceinline__ PairRow pair_row(const PairArgs& a, int k, int N) {
    PairRow r;
    r.sig = PACKED ? k : a.table[2 * (size_t)k];
    r.f0 = PACKED ? 0 : a.table[2 * (size_t)k + 1];
    r.nf = r.len_x = r.len_y = 0;
    r.orow = PACKED ? 0 : (int64_t)k * a.T;
    if (r.sig < 0 || r.sig >= a.n_sig || r.f0 < 0) {
        r.sig = -1;
        return r;
    }
    int64_t ly = a.len_y[r.sig], lx = a.len_x[r.sig];
    r.len_y = ly < 0 ? 0 : (ly > a.stride_y ? a.stride_y : ly);
    r.len_x = lx < 0 ? 0 : (lx > a.stride_x ? a.stride_x : lx);
    // written out, not stft_frame_count: through the call the PACKED kernels come out with other instructions
    const int64_t nfram = (r.len_y + a.hop - 1) / a.hop;          // as drnmf_stft_frames
    r.nf = 1 + (nfram * a.hop + (int64_t)N) / a.hop;
    if (PACKED) {
        r.orow = a.row0[r.sig];
        // rows outside [0, total_frames) are not written: a row0 that is not the prefix sum loses frames,
        // it never writes past the buffers
        if (r.orow < 0) r.sig = -1;
        else if (r.nf > a.total_frames - r.orow) r.nf = a.total_frames - r.orow;
    }
    return r;
}

// 0: t holds frame f0 + t of the signal; 1: a padding frame (chunks only); 2: nothing is written
template <bool PACKED>
__device__ __forceinline__ int pair_state(const PairRow& r, int64_t t, int T) {
    if (t >= T) return 2;
    if (r.sig >= 0 && r.f0 + t < r.nf) return 0;
    return PACKED ? 2 : 1;
}

// The frames of a workgroup of the fast path: tw [N/2] and bufs [4][MP] are the kernel's LDS, tg its PairTarget
// (stft_pair_target_real_kernel) or a NoTarget (stft_pair_real_kernel).
template <int R, int P, bool PACKED, class TG>
__device__ __forceinline__ void pair_real_frames(const PairArgs& a, float2* tw, float2 (*bufs)[RealFft<R, P>::MP],
                                                 TG* tg) {
    constexpr int N = RealFft<R, P>::N, F = N / 2 + 1;
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    const int64_t t0 = ((int64_t)blockIdx.x + a.tile_base) * 4, t = t0 + wv;
    const int k = (int)blockIdx.y + a.row_base;
    const PairRow row = pair_row<PACKED>(a, k, N);
    // the states of a row are 0 up to some t and not 0 behind it: a tile whose first frame is no frame holds
    // none, and stages nothing (the whole workgroup takes this branch: no barrier is skipped by a part of it)
    if (pair_state<PACKED>(row, t0, a.T) == 0) {
        for (int i = tid; i < N / 2; i += 256) tw[i] = g_twiddle[a.logN - TAB_LOG_MIN][i];
        __syncthreads();
    }
    const int st = pair_state<PACKED>(row, t, a.T);
    if (st == 2) return;                      // (whole waves: no barrier below)
    const size_t o = (size_t)(row.orow + t) * F;
    if (st == 1) {                            // padding frame: Masking's value in every bin, weight 0
        for (int i = j; i < F; i += 64) {
            a.x[o + i] = a.mask_value;
            a.y[o + i] = a.mask_value;
        }
        if (j == 0) a.w[row.orow + t] = 0.f;
        return;
    }
    const int frame = (int)(row.f0 + t);
    // ONE copy of the frame body, run for the noisy and then for the clean member (the loop is kept a loop): both
    // sides execute the same instructions, those of a kernel that holds the body once -- two inlined copies are
    // free to contract their multiply-adds differently, and then differ from drnmf_stft in the last bit
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
        const void* pcm = side ? a.pcm_y : a.pcm_x;
        const int64_t stride = side ? a.stride_y : a.stride_x, len = side ? row.len_y : row.len_x;
        if constexpr (TG::on) tg->side = side;
        stft_real_frame<R, P>(pcm, a.is_int16, (size_t)row.sig * stride, len, a.logN, a.hop, frame, o,
                              side ? a.y : a.x, a.re, a.im, tw, bufs[wv], j, a.transform, tg);
        // the wave's LDS slice is reused: its reads of this spectrum are issued before the next member's writes,
        // and LDS serves one wave's requests in order (as between the passes of stockham_passes)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (!PACKED && j == 0) a.w[row.orow + t] = 1.f;
}

template <int R, int P, bool PACKED>
__global__ void __launch_bounds__(256) stft_pair_real_kernel(const PairArgs a) {
    __shared__ float2 tw[RealFft<R, P>::N / 2];
    __shared__ float2 bufs[4][RealFft<R, P>::MP];
    NoTarget none;
    pair_real_frames<R, P, PACKED>(a, tw, bufs, &none);
}

// the same with y = the 'psa' / 'tpsa' target (drnmf_stft_pair_chunks_target; x and w as above, bit for bit)
template <int R, int P>
__global__ void __launch_bounds__(256) stft_pair_target_real_kernel(const PairArgs a, int target) {
    __shared__ float2 tw[RealFft<R, P>::N / 2];
    __shared__ float2 bufs[4][RealFft<R, P>::MP];
    PairTarget<RealFft<R, P>::M / 64 + 1> tg;
    tg.target = target;
    pair_real_frames<R, P, false>(a, tw, bufs, &tg);
}

// other sizes: one workgroup per (row, frame), the noisy frame and then the clean one through the same buffer
// (smem: the kernel's dynamic LDS, N points and N/2 twiddles)
template <bool PACKED, class TG>
__device__ __forceinline__ void pair_frame(const PairArgs& a, int N, float* smem, TG* tg) {
    float2* buf = (float2*)smem;
    float2* tw = buf + N;
    const int tid = threadIdx.x, F = N / 2 + 1;
    const int64_t t = (int64_t)blockIdx.x + a.tile_base;
    const int k = (int)blockIdx.y + a.row_base;
    const PairRow row = pair_row<PACKED>(a, k, N);
    const int st = pair_state<PACKED>(row, t, a.T);       // (uniform over the workgroup, as both exits below)
    if (st == 2) return;
    const size_t o = (size_t)(row.orow + t) * F;
    if (st == 1) {
        for (int i = tid; i < F; i += 256) {
            a.x[o + i] = a.mask_value;
            a.y[o + i] = a.mask_value;
        }
        if (tid == 0) a.w[row.orow + t] = 0.f;
        return;
    }
    const int frame = (int)(row.f0 + t);
    for (int k = tid; k < N / 2; k += 256) tw[k] = g_twiddle[a.logN - TAB_LOG_MIN][k];    // once per pair
    // one copy of the frame body for both members, as in the kernel above
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
        const void* pcm = side ? a.pcm_y : a.pcm_x;
        const int64_t stride = side ? a.stride_y : a.stride_x, len = side ? row.len_y : row.len_x;
        if constexpr (TG::on) tg->side = side;
        stft_frame(pcm, a.is_int16, (size_t)row.sig * stride, len, N, a.logN, a.hop, frame, o, side ? a.y : a.x,
                   a.re, a.im, buf, tw, tid, a.transform, false, tg);
        __syncthreads();                      // this spectrum has been read out of buf
    }
    if (!PACKED && tid == 0) a.w[row.orow + t] = 1.f;
}

template <bool PACKED>
__global__ void __launch_bounds__(256) stft_pair_kernel(const PairArgs a, int N) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    NoTarget none;
    pair_frame<PACKED>(a, N, smem, &none);
}

// the target sibling: thread tid holds bins tid + 256 s, s < 9 (F <= 2049)
__global__ void __launch_bounds__(256) stft_pair_target_kernel(const PairArgs a, int N, int target) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    PairTarget<TAB_N_MAX / 2 / 256 + 1> tg;
    tg.target = target;
    pair_frame<false>(a, N, smem, &tg);
}

// ---------------------------------------------------------------------------------------------
// Transpose of the ragged masked inverse (include/drnmf_waveloss.h): the frame bodies above run on the waveform
// cotangent g, and the epilogue multiplies each bin of G with the stored spectrum instead of writing it:
//   d_mask[k] = (c_k / N) (2 hop / N) (re[k] Re G[k] + im[k] Im G[k]),  c_0 = c_{N/2} = 1, else 2.
// The bodies hand a bin over as PairTarget receives it (re_k, im_k in the stored, conjugated convention); a lane's
// slot s is bin lane + STEP s in both bodies (the wave body's extra slot M/64 of lane 0 is bin M).  Nothing of G
// goes through memory, and the magnitude the bodies compute beside it is dead code here.
template <int SLOTS, int STEP>
struct VjpBin {
    static constexpr bool on = true;
    static constexpr int slots = SLOTS;
    const float* re;              // the frame's stored spectrum rows
    const float* im;
    int lane, half;               // half = N/2
    float coef;                   // (1 / N) (2 hop / N)
    __device__ __forceinline__ float bin(int s, float re_k, float im_k, float, float) const {
        const int k = lane + STEP * s;
        const float c = (k == 0 || k == half) ? coef : 2.f * coef;
        return c * (re[k] * re_k + im[k] * im_k);
    }
};

// what a workgroup of either kernel knows of slab row k: the row, the samples of g that count and the frames
struct VjpRow {
    RaggedRow row;
    int64_t nout, nfe;
};

__device__ __forceinline__ VjpRow vjp_row(const int64_t* __restrict__ lengths, const int* __restrict__ sig_index,
                                          int n_sig, int k, int T, int N, int hop, int crop, int64_t ld_g) {
    VjpRow v;
    v.row = ragged_row(lengths, sig_index, n_sig, k, (int64_t)1 << 40, N, hop);      // as the inverse clamps
    v.nout = v.row.sig < 0 ? 0 : ragged_nout(v.row, N, hop, crop, ld_g);
    v.nfe = v.row.nf < T ? v.row.nf : T;
    return v;
}

template <int R, int P>
__global__ void __launch_bounds__(256)
istft_vjp_real_kernel(const float* __restrict__ g, int64_t ld_g, const int64_t* __restrict__ lengths,
                      const int* __restrict__ sig_index, int n_sig, int T, int logN, int hop, int crop,
                      const float* __restrict__ re, const float* __restrict__ im, float* __restrict__ d_mask,
                      int64_t ld_dm) {
    constexpr int M = RealFft<R, P>::M, N = 2 * M, F = M + 1;
    __shared__ float2 tw[N / 2];
    __shared__ float2 bufs[4][RealFft<R, P>::MP];
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    const int frame = blockIdx.x * 4 + wv, k = blockIdx.y;
    for (int i = tid; i < N / 2; i += 256) tw[i] = g_twiddle[logN - TAB_LOG_MIN][i];
    __syncthreads();
    if (frame >= T) return;                   // (whole waves: no barrier below)
    const VjpRow v = vjp_row(lengths, sig_index, n_sig, k, T, N, hop, crop, ld_g);
    const size_t fr = (size_t)k * T + frame, o = fr * (size_t)ld_dm;
    if (frame >= v.nfe) {                     // no frame of this row: its mask never reached a sample
        for (int64_t i = j; i < ld_dm; i += 64) d_mask[o + i] = 0.f;
        return;
    }
    for (int64_t i = F + j; i < ld_dm; i += 64) d_mask[o + i] = 0.f;
    VjpBin<M / 64 + 1, 64> tg{re + fr * F, im + fr * F, j, M,
                              (2.0f / ((float)N / (float)hop)) / (float)N};
    stft_real_frame<R, P>(g, 0, (size_t)v.row.sig * ld_g, v.nout, logN, hop, frame, o, d_mask, nullptr, nullptr,
                          tw, bufs[wv], j, 0, &tg);
}

// other sizes: one workgroup per (row, frame); thread tid holds bins tid + 256 s, s < 9 (F <= 2049)
__global__ void __launch_bounds__(256)
istft_vjp_kernel(const float* __restrict__ g, int64_t ld_g, const int64_t* __restrict__ lengths,
                 const int* __restrict__ sig_index, int n_sig, int T, int N, int logN, int hop, int crop,
                 const float* __restrict__ re, const float* __restrict__ im, float* __restrict__ d_mask,
                 int64_t ld_dm) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float2* buf = (float2*)smem;
    float2* tw = buf + N;
    const int tid = threadIdx.x, frame = blockIdx.x, k = blockIdx.y, F = N / 2 + 1;
    const VjpRow v = vjp_row(lengths, sig_index, n_sig, k, T, N, hop, crop, ld_g);
    const size_t fr = (size_t)k * T + frame, o = fr * (size_t)ld_dm;
    if (frame >= v.nfe) {                     // (the whole workgroup: no barrier is skipped by a part of it)
        for (int64_t i = tid; i < ld_dm; i += 256) d_mask[o + i] = 0.f;
        return;
    }
    for (int64_t i = F + tid; i < ld_dm; i += 256) d_mask[o + i] = 0.f;
    VjpBin<TAB_N_MAX / 2 / 256 + 1, 256> tg{re + fr * F, im + fr * F, tid, N / 2,
                                            (2.0f / ((float)N / (float)hop)) / (float)N};
    stft_frame(g, 0, (size_t)v.row.sig * ld_g, v.nout, N, logN, hop, frame, o, d_mask, nullptr, nullptr, buf, tw,
               tid, 0, true, &tg);
}

}  // namespace

extern "C" int32_t drnmf_stft_frames(int64_t nsampl, int32_t N, int32_t hop) {
    if (nsampl < 0 || N <= 0 || hop <= 0) return -1;
    return (int32_t)stft_frame_count(nsampl, N, hop);
}

// drnmf_stft_mag (re = im = NULL) and drnmf_stft (mag may be NULL) behind their own checks
static int32_t enqueue_stft(drnmf_handle_t h, int32_t n_sig, int64_t nsampl, int32_t N, int32_t hop,
                            int32_t is_int16, const void* pcm, float* mag, float* re, float* im, void* stream_) {
    FftCall c;
    if (const int32_t rc = fft_call(h, N, stream_, &c)) return rc;
    const int nf = drnmf_stft_frames(nsampl, N, hop);
    with_fft_size(N, [&](auto s) {
        using S = decltype(s);
        if constexpr (S::fast)
            hipLaunchKernelGGL((stft_real_kernel<S::R, S::P>), dim3((unsigned)((nf + 3) / 4), (unsigned)n_sig),
                               dim3(256), 0, c.stream, pcm, is_int16, nsampl, c.logN, hop, nf, mag, re, im);
        else
            hipLaunchKernelGGL(stft_kernel, dim3((unsigned)nf, (unsigned)n_sig), dim3(256), c.lds, c.stream, pcm,
                               is_int16, nsampl, N, c.logN, hop, nf, mag, re, im);
    });
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

extern "C" int32_t drnmf_stft_mag(drnmf_handle_t h, int32_t n_sig, int64_t nsampl, int32_t N,
                                  int32_t hop, int32_t is_int16, const void* pcm, float* mag,
                                  void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (n_sig <= 0 || nsampl <= 0 || hop <= 0)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "stft_mag: bad shape n_sig=%d nsampl=%lld hop=%d",
                   n_sig, (long long)nsampl, hop);
    if (const int32_t rc = check_fft_size(h, "stft_mag", N, DRNMF_ERR_UNSUPPORTED)) return rc;
    if (!pcm || !mag) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "stft_mag: NULL pointer argument");
    return enqueue_stft(h, n_sig, nsampl, N, hop, is_int16, pcm, mag, nullptr, nullptr, stream_);
}

extern "C" int32_t drnmf_stft(drnmf_handle_t h, int32_t n_sig, int64_t nsampl, int32_t N,
                              int32_t hop, int32_t is_int16, const void* pcm, float* re, float* im,
                              float* mag, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (n_sig <= 0 || nsampl <= 0 || hop <= 0 || !pcm || !re || !im)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "stft: bad argument");
    if (const int32_t rc = check_fft_size(h, "stft", N, DRNMF_ERR_UNSUPPORTED)) return rc;
    return enqueue_stft(h, n_sig, nsampl, N, hop, is_int16, pcm, mag, re, im, stream_);
}

extern "C" size_t drnmf_istft_workspace_bytes(int32_t n_sig, int32_t n_frames, int32_t N) {
    if (n_sig <= 0 || n_frames <= 0 || N <= 0) return 0;
    return round_up_sz((size_t)n_sig * n_frames * N * sizeof(float), 256);
}

extern "C" int32_t drnmf_istft_masked(drnmf_handle_t h, int32_t n_sig, int32_t n_frames,
                                      int64_t nsampl, int32_t N, int32_t hop, const float* re,
                                      const float* im, const float* mask, float* y,
                                      void* workspace, size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (n_sig <= 0 || n_frames <= 0 || nsampl <= 0 || hop <= 0 || !re || !im || !y || !workspace)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "istft_masked: bad argument");
    if (const int32_t rc = check_fft_size(h, "istft_masked", N, DRNMF_ERR_UNSUPPORTED)) return rc;
    if (workspace_bytes < drnmf_istft_workspace_bytes(n_sig, n_frames, N))
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "istft_masked: workspace too small");
    FftCall c;
    if (const int32_t rc = fft_call(h, N, stream_, &c)) return rc;
    float* frames = (float*)workspace;
    // every size takes the radix-2 inverse: this entry has no fused kernel
    hipLaunchKernelGGL(istft_frames_kernel, dim3((unsigned)n_frames, (unsigned)n_sig), dim3(256), c.lds, c.stream,
                       re, im, mask, N, c.logN, hop, n_frames, frames);
    hipLaunchKernelGGL(overlap_add_kernel, dim3((unsigned)((nsampl + 255) / 256), (unsigned)n_sig),
                       dim3(256), 0, c.stream, frames, N, hop, n_frames, nsampl, y);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

extern "C" int32_t drnmf_snr(drnmf_handle_t h, int32_t n_sig, int64_t nsampl, const float* est,
                             const float* ref, float* out_db, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (n_sig <= 0 || nsampl <= 0 || !est || !ref || !out_db)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "snr: bad argument");
    hipLaunchKernelGGL(snr_kernel, dim3((unsigned)n_sig), dim3(256), 0, (hipStream_t)stream_, est,
                       ref, nsampl, out_db);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

// ---- ragged batches (include/drnmf_enhance.h) ------------------------------------------------------------
static bool istft_ragged_fused(int N, int hop) { return stft_fast(N) && hop <= N; }

static int ragged_run(int hop) {              // samples per workgroup of the fused inverse: C hop <= 2048
    const int C = 2048 / hop;
    return (C < 1 ? 1 : C) * hop;
}

extern "C" int32_t drnmf_stft_ragged(drnmf_handle_t h, int32_t n_sig, int64_t stride, const int64_t* lengths,
                                     int32_t b, const int32_t* sig_index, int32_t T, int32_t N, int32_t hop,
                                     int32_t is_int16, float mask_value, const void* pcm, float* x, float* re,
                                     float* im, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (n_sig <= 0 || stride <= 0 || b <= 0 || b > 65535 || T <= 0 || hop <= 0)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG,
                   "stft_ragged: bad shape n_sig=%d stride=%lld b=%d (1..65535) T=%d hop=%d", n_sig,
                   (long long)stride, b, T, hop);
    if (const int32_t rc = check_fft_size(h, "stft_ragged", N, DRNMF_ERR_INVALID_ARG)) return rc;
    if (!lengths || !sig_index || !pcm || !x || !re || !im)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "stft_ragged: NULL pointer argument");
    FftCall c;
    if (const int32_t rc = fft_call(h, N, stream_, &c)) return rc;
    with_fft_size(N, [&](auto s) {
        using S = decltype(s);
        if constexpr (S::fast)
            hipLaunchKernelGGL((stft_real_ragged_kernel<S::R, S::P>), dim3((unsigned)((T + 3) / 4), (unsigned)b),
                               dim3(256), 0, c.stream, pcm, is_int16, stride, lengths, sig_index, n_sig, T, c.logN,
                               hop, mask_value, x, re, im);
        else
            hipLaunchKernelGGL(stft_ragged_kernel, dim3((unsigned)T, (unsigned)b), dim3(256), c.lds, c.stream, pcm,
                               is_int16, stride, lengths, sig_index, n_sig, T, N, c.logN, hop, mask_value, x, re,
                               im);
    });
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

extern "C" size_t drnmf_istft_ragged_workspace_bytes(int32_t b, int32_t T, int32_t N, int32_t hop) {
    if (b <= 0 || T <= 0 || N <= 0 || hop <= 0 || istft_ragged_fused(N, hop)) return 0;
    return round_up_sz((size_t)b * T * N * sizeof(float), 256);
}

extern "C" int32_t drnmf_istft_ragged(drnmf_handle_t h, int32_t n_sig, int32_t b, int32_t T, int32_t N,
                                      int32_t hop, const int64_t* lengths, const int32_t* sig_index,
                                      const float* re, const float* im, const float* mask, int64_t ld_mask,
                                      float* y, int64_t stride_y, int32_t crop, void* workspace,
                                      size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (n_sig <= 0 || b <= 0 || b > 65535 || T <= 0 || hop <= 0 || stride_y <= 0 || (crop != 0 && crop != 1))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG,
                   "istft_ragged: bad shape n_sig=%d b=%d (1..65535) T=%d hop=%d stride_y=%lld crop=%d", n_sig,
                   b, T, hop, (long long)stride_y, crop);
    if (const int32_t rc = check_fft_size(h, "istft_ragged", N, DRNMF_ERR_INVALID_ARG)) return rc;
    if (!lengths || !sig_index || !re || !im || !y)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "istft_ragged: NULL pointer argument");
    if (mask && ld_mask < N / 2 + 1)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "istft_ragged: ld_mask=%lld is below N/2+1=%d",
                   (long long)ld_mask, N / 2 + 1);
    const size_t need = drnmf_istft_ragged_workspace_bytes(b, T, N, hop);
    if (need && (!workspace || workspace_bytes < need))
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "istft_ragged: workspace too small (%zu < %zu bytes)",
                   workspace ? workspace_bytes : (size_t)0, need);
    FftCall c;
    if (const int32_t rc = fft_call(h, N, stream_, &c)) return rc;
    const bool fused = istft_ragged_fused(N, hop);        // the rule drnmf_istft_ragged_workspace_bytes answers from
    with_fft_size(N, [&](auto s) {
        using S = decltype(s);
        if constexpr (S::fast) {
            if (fused) {
                const int run = ragged_run(hop);
                hipLaunchKernelGGL((istft_real_ragged_kernel<S::R, S::P>),
                                   dim3((unsigned)((stride_y + run - 1) / run), (unsigned)b), dim3(256), 0, c.stream,
                                   re, im, mask, ld_mask, lengths, sig_index, n_sig, T, c.logN, hop, run, crop, y,
                                   stride_y);
                return;
            }
        }
        float* frames = (float*)workspace;
        hipLaunchKernelGGL(istft_frames_ragged_kernel, dim3((unsigned)T, (unsigned)b), dim3(256), c.lds, c.stream,
                           re, im, mask, ld_mask, lengths, sig_index, n_sig, T, N, c.logN, hop, frames);
        hipLaunchKernelGGL(overlap_add_ragged_kernel, dim3((unsigned)((stride_y + 255) / 256), (unsigned)b),
                           dim3(256), 0, c.stream, frames, lengths, sig_index, n_sig, T, N, hop, crop, y, stride_y);
    });
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

// include/drnmf_waveloss.h: every size is one launch of a frame body with the VjpBin epilogue
extern "C" int32_t drnmf_istft_ragged_vjp(drnmf_handle_t h, int32_t n_sig, int32_t b, int32_t T, int32_t N,
                                          int32_t hop, const int64_t* lengths, const int32_t* sig_index,
                                          const float* re, const float* im, const float* g, int64_t ld_g,
                                          int32_t crop, float* d_mask, int64_t ld_dm, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (n_sig <= 0 || b <= 0 || b > 65535 || T <= 0 || hop <= 0 || ld_g <= 0 || (crop != 0 && crop != 1))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG,
                   "istft_ragged_vjp: bad shape n_sig=%d b=%d (1..65535) T=%d hop=%d ld_g=%lld crop=%d", n_sig, b,
                   T, hop, (long long)ld_g, crop);
    if (const int32_t rc = check_fft_size(h, "istft_ragged_vjp", N, DRNMF_ERR_INVALID_ARG)) return rc;
    if (!lengths || !sig_index || !re || !im || !g || !d_mask)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "istft_ragged_vjp: NULL pointer argument");
    if (ld_dm < N / 2 + 1)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "istft_ragged_vjp: ld_dm=%lld is below N/2+1=%d", (long long)ld_dm,
                   N / 2 + 1);
    FftCall c;
    if (const int32_t rc = fft_call(h, N, stream_, &c)) return rc;
    with_fft_size(N, [&](auto s) {
        using S = decltype(s);
        if constexpr (S::fast)
            hipLaunchKernelGGL((istft_vjp_real_kernel<S::R, S::P>), dim3((unsigned)((T + 3) / 4), (unsigned)b),
                               dim3(256), 0, c.stream, g, ld_g, lengths, sig_index, n_sig, T, c.logN, hop, crop, re,
                               im, d_mask, ld_dm);
        else
            hipLaunchKernelGGL(istft_vjp_kernel, dim3((unsigned)T, (unsigned)b), dim3(256), c.lds, c.stream, g, ld_g,
                               lengths, sig_index, n_sig, T, N, c.logN, hop, crop, re, im, d_mask, ld_dm);
    });
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

// ---- paired training tensors (include/drnmf_dataset.h) ----------------------------------------------------
// Rows (sequences, or signals in the packed mode) go on grid.y in slices of at most 65535 and frame tiles on
// grid.x in slices of at most 2^23, so neither count is bounded by a grid dimension.
template <bool PACKED>
static void launch_stft_pair(PairArgs a, const FftCall& c, int64_t n_rows, int target = DRNMF_TARGET_MAG) {
    const int N = c.N;
    const int64_t tiles = stft_fast(N) ? ((int64_t)a.T + 3) / 4 : (int64_t)a.T;
    const int64_t max_y = 65535, max_x = (int64_t)1 << 23;
    for (int64_t r0 = 0; r0 < n_rows; r0 += max_y)
        for (int64_t x0 = 0; x0 < tiles; x0 += max_x) {
            a.row_base = (int)r0;
            a.tile_base = (int)x0;
            const dim3 grid((unsigned)(tiles - x0 < max_x ? tiles - x0 : max_x),
                            (unsigned)(n_rows - r0 < max_y ? n_rows - r0 : max_y));
            with_fft_size(N, [&](auto s) {
                using S = decltype(s);
                if (!PACKED && target != DRNMF_TARGET_MAG) {
                    if constexpr (S::fast)
                        hipLaunchKernelGGL((stft_pair_target_real_kernel<S::R, S::P>), grid, dim3(256), 0, c.stream,
                                           a, target);
                    else
                        hipLaunchKernelGGL(stft_pair_target_kernel, grid, dim3(256), c.lds, c.stream, a, N, target);
                } else if constexpr (S::fast)
                    hipLaunchKernelGGL((stft_pair_real_kernel<S::R, S::P, PACKED>), grid, dim3(256), 0, c.stream, a);
                else
                    hipLaunchKernelGGL((stft_pair_kernel<PACKED>), grid, dim3(256), c.lds, c.stream, a, N);
            });
        }
}

// the arguments both entry points share; 0 or a status with the handle's message set
static int32_t check_stft_pair(drnmf_handle_t h, const char* who, int32_t n_sig, int64_t stride_x,
                               int64_t stride_y, int32_t N, int32_t hop, int32_t is_int16, int32_t transform) {
    if (n_sig <= 0 || stride_x <= 0 || stride_y <= 0 || hop <= 0 || (is_int16 != 0 && is_int16 != 1))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG,
                   "%s: bad shape n_sig=%d stride_x=%lld stride_y=%lld hop=%d is_int16=%d", who, n_sig,
                   (long long)stride_x, (long long)stride_y, hop, is_int16);
    if (const int32_t rc = check_fft_size(h, who, N, DRNMF_ERR_INVALID_ARG)) return rc;
    if (transform != DRNMF_TRANSFORM_MAG && transform != DRNMF_TRANSFORM_LOGMAG)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: transform=%d is neither DRNMF_TRANSFORM_MAG nor _LOGMAG", who,
                   transform);
    if (stride_y / hop + N / hop + 2 > 0x7fffffff)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: stride_y=%lld at hop=%d has more than 2^31-1 frames", who,
                   (long long)stride_y, hop);
    return DRNMF_OK;
}

// the argument checks of drnmf_stft_pair_chunks and drnmf_stft_pair_chunks_target (who), then their enqueue
static int32_t check_stft_pair_chunks(drnmf_handle_t h, const char* who, int32_t n_sig, int64_t stride_x,
                                      int64_t stride_y, const int64_t* len_x, const int64_t* len_y, int32_t n_seq,
                                      const int32_t* seq_table, int32_t T, int32_t N, int32_t hop,
                                      int32_t is_int16, int32_t transform, const void* pcm_x, const void* pcm_y,
                                      const float* x, const float* y, const float* w) {
    if (n_seq <= 0 || T <= 0) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: bad shape n_seq=%d T=%d", who, n_seq, T);
    const int32_t rc = check_stft_pair(h, who, n_sig, stride_x, stride_y, N, hop, is_int16, transform);
    if (rc) return rc;
    if (!len_x || !len_y || !seq_table || !pcm_x || !pcm_y || !x || !y || !w)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: NULL pointer argument", who);
    return DRNMF_OK;
}

static int32_t enqueue_stft_pair_chunks(drnmf_handle_t h, int32_t n_sig, int64_t stride_x, int64_t stride_y,
                                        const int64_t* len_x, const int64_t* len_y, int32_t n_seq,
                                        const int32_t* seq_table, int32_t T, int32_t N, int32_t hop,
                                        int32_t is_int16, int32_t transform, int32_t target, float mask_value,
                                        const void* pcm_x, const void* pcm_y, float* x, float* y, float* w,
                                        void* stream_) {
    FftCall c;
    if (const int32_t rc = fft_call(h, N, stream_, &c)) return rc;
    PairArgs a = {pcm_x, pcm_y, len_x, len_y, stride_x, stride_y, seq_table, nullptr, 0, x, y, w,
                  nullptr, nullptr, n_sig, T, hop, c.logN, is_int16, transform, mask_value, 0, 0};
    launch_stft_pair<false>(a, c, n_seq, target);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

extern "C" int32_t drnmf_stft_pair_chunks(drnmf_handle_t h, int32_t n_sig, int64_t stride_x, int64_t stride_y,
                                          const int64_t* len_x, const int64_t* len_y, int32_t n_seq,
                                          const int32_t* seq_table, int32_t T, int32_t N, int32_t hop,
                                          int32_t is_int16, int32_t transform, float mask_value,
                                          const void* pcm_x, const void* pcm_y, float* x, float* y, float* w,
                                          void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    const int32_t rc = check_stft_pair_chunks(h, "stft_pair_chunks", n_sig, stride_x, stride_y, len_x, len_y, n_seq,
                                              seq_table, T, N, hop, is_int16, transform, pcm_x, pcm_y, x, y, w);
    if (rc) return rc;
    return enqueue_stft_pair_chunks(h, n_sig, stride_x, stride_y, len_x, len_y, n_seq, seq_table, T, N, hop,
                                    is_int16, transform, DRNMF_TARGET_MAG, mask_value, pcm_x, pcm_y, x, y, w, stream_);
}

// include/drnmf_target.h
extern "C" int32_t drnmf_stft_pair_chunks_target(drnmf_handle_t h, int32_t n_sig, int64_t stride_x,
                                                 int64_t stride_y, const int64_t* len_x, const int64_t* len_y,
                                                 int32_t n_seq, const int32_t* seq_table, int32_t T, int32_t N,
                                                 int32_t hop, int32_t is_int16, int32_t transform, int32_t target,
                                                 float mask_value, const void* pcm_x, const void* pcm_y, float* x,
                                                 float* y, float* w, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    const char* who = "stft_pair_chunks_target";
    if (target != DRNMF_TARGET_MAG && target != DRNMF_TARGET_PSA && target != DRNMF_TARGET_TPSA)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: target=%d is none of DRNMF_TARGET_MAG, _PSA, _TPSA", who, target);
    const int32_t rc = check_stft_pair_chunks(h, who, n_sig, stride_x, stride_y, len_x, len_y, n_seq, seq_table, T,
                                              N, hop, is_int16, transform, pcm_x, pcm_y, x, y, w);
    if (rc) return rc;
    if (target != DRNMF_TARGET_MAG && transform != DRNMF_TRANSFORM_MAG)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: target=%d is defined for DRNMF_TRANSFORM_MAG only (transform=%d)",
                   who, target, transform);
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "%s: the handle is bound to no device", who);
    return enqueue_stft_pair_chunks(h, n_sig, stride_x, stride_y, len_x, len_y, n_seq, seq_table, T, N, hop,
                                    is_int16, transform, target, mask_value, pcm_x, pcm_y, x, y, w, stream_);
}

extern "C" int32_t drnmf_stft_pair_frames(drnmf_handle_t h, int32_t n_sig, int64_t stride_x, int64_t stride_y,
                                          const int64_t* len_x, const int64_t* len_y, const int64_t* row0,
                                          int64_t total_frames, int32_t N, int32_t hop, int32_t is_int16,
                                          int32_t transform, const void* pcm_x, const void* pcm_y,
                                          float* x_frames, float* y_frames, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (total_frames <= 0)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "stft_pair_frames: bad shape total_frames=%lld",
                   (long long)total_frames);
    const int32_t rc = check_stft_pair(h, "stft_pair_frames", n_sig, stride_x, stride_y, N, hop, is_int16,
                                       transform);
    if (rc) return rc;
    if (!len_x || !len_y || !row0 || !pcm_x || !pcm_y || !x_frames || !y_frames)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "stft_pair_frames: NULL pointer argument");
    FftCall c;
    if (const int32_t rc = fft_call(h, N, stream_, &c)) return rc;
    // the grid spans the frames the longest signal can have; a signal's own count is evaluated on the device
    const int T = drnmf_stft_frames(stride_y, N, hop);
    PairArgs a = {pcm_x, pcm_y, len_x, len_y, stride_x, stride_y, nullptr, row0, total_frames, x_frames,
                  y_frames, nullptr, nullptr, nullptr, n_sig, T, hop, c.logN, is_int16, transform, 0.f, 0, 0};
    launch_stft_pair<true>(a, c, n_sig);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

// ---- streaming (include/drnmf_stream.h) -------------------------------------------------------------------
#include "stft_stream.h"
