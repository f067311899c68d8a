// Device-side rational-rate resampler (include/drnmf_resample.h): a ragged batch of waveforms through one polyphase
// FIR pass, y[m] = sum_k x[k] h[q m + half - p k], each output one ascending fp64 fma chain rounded once to float32.
// About 2 nz max(1, q / p) terms per output against 4 bytes written and 4 q / p read: the samples are touched once
// in global memory, the work is LDS reads.
//
// A workgroup of 1024 threads owns one tile of outputs of one signal (grid.x: tiles, grid.y: signals in slices of at
// most 65535).  It stages the WHOLE filter (fp64, L = 2 nz max(p, q) + 1 taps: 100 KB at max(p, q) = 640) and the
// tile's input span (float32; int16 converted here) in LDS once, then thread t sums the outputs t, t + 1024, ... of
// the tile.  The LDS of a launch is the table plus the span, so 48000 -> 16000 (61 taps, 25 KB of samples) puts six
// workgroups on a compute unit and 44100 -> 16000 (8821 taps, 70 KB) one -- hence 1024 threads: four waves per SIMD
// hide the latency of the dependent chain.  A tile is 2048 outputs; where the span of 2048 outputs would not fit
// beside the table (decimation by 20 and more) it is as many outputs as fit (resample_plan): 4 at p / q = 1 / 640.
//
// LDS banks.  In step c of their chains the lanes of a wave read taps (L - 1 - e_m) - p c with e_m = (half - q m)
// mod p, m the lane's output: one address for p = 1 (a broadcast), and for p a multiple of 32 the residues of q m
// mod 32 of 32 consecutive m are distinct whenever q is odd -- 160 / 441 and 640 / 441 read without conflicts, 441 /
// 160 meets about three lanes per bank.  The samples are read at stride q / p.
//
// The chunked form (drnmf_resample_chunk) is the same kernel: a row holds a window of its signal that starts at
// sample in_start, and the outputs written start at out_start; every index below is global, only the staging
// subtracts in_start.  p == q == 1 is resample_copy_kernel, which shares the window arithmetic and reads no filter.
#include <atomic>

#include "common.h"
#include "resample_filter.h"
#include "../../include/drnmf_resample.h"

namespace {

constexpr int THREADS = 1024;
constexpr int TILE = DRNMF_RESAMPLE_TILE;
constexpr int MAX_PQ = DRNMF_RESAMPLE_MAX_PQ;
constexpr int MAX_NZ = 1024;                        // keeps L inside an int; LDS refuses far earlier
constexpr int64_t LDS_BYTES = 160 * 1024;           // a compute unit's; one workgroup may take all of it
constexpr int64_t MAX_STRIDE = (int64_t)1 << 40;
constexpr int64_t MAX_INDEX = (int64_t)1 << 50;     // a global sample / output index: q * index stays inside an int64
constexpr int CARRY_BLOCK = 4096;                   // elements per workgroup of the carry kernel

struct Plan {
    int L, half, tile, span;       // taps, (L - 1) / 2, outputs per workgroup, samples staged per workgroup at most
    size_t lds;
};

// the samples a tile of t outputs can meet: the integers k with lo <= p k <= hi, hi - lo = q (t - 1) + L - 1, and one
static int64_t tile_span(int p, int q, int L, int64_t t) { return ((int64_t)q * (t - 1) + L - 1) / p + 2; }

static bool resample_plan(int p, int q, int nz, Plan* pl) {
    if (p < 1 || q < 1 || p > MAX_PQ || q > MAX_PQ || nz < 1 || nz > MAX_NZ) return false;
    const int L = 2 * nz * (p > q ? p : q) + 1;
    const int64_t cap = (LDS_BYTES - 8 * (int64_t)L) / 4;      // floats beside the table
    if (cap < 3) return false;
    int64_t t = TILE;
    if (tile_span(p, q, L, t) > cap) {
        const int64_t room = (cap - 1) * p - 1 - (L - 1);      // floor((q (t - 1) + L - 1) / p) <= cap - 2
        if (room < 0) return false;
        t = room / q + 1;
    }
    pl->L = L;
    pl->half = (L - 1) / 2;
    pl->tile = (int)t;
    pl->span = (int)tile_span(p, q, L, t);
    pl->lds = round_up_sz(8 * (size_t)L + 4 * (size_t)pl->span, 16);
    return true;
}

static int64_t gcd_i64(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

__device__ __forceinline__ int64_t clamp_i64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool I16>
__device__ __forceinline__ float sample_at(const void* __restrict__ row, int64_t m) {
    if constexpr (I16)
        return (float)((const short*)row)[m] / 32768.0f;      // as mix.hip and reverb.hip read int16
    else
        return ((const float*)row)[m];
}

struct ResampleArgs {
    const void* in;
    const double* taps;
    const int64_t* len;
    const int64_t* in_start;    // or NULL: 0
    const int64_t* out_start;   // or NULL: 0
    const int64_t* out_count;   // or NULL: every output from out_start on
    const int64_t* total;       // or NULL: len
    float* out;
    int64_t stride_in, stride_out;
    int p, q, L, tile, span, sig_base;
};

// What row i holds and what the call writes of it, in global indices: samples [in0, n) of the signal (n already cut
// at the signal's end where that is known), outputs o0 .. o0 + cnt - 1 to out[i][0 .. cnt).
struct Window {
    int64_t in0, n, o0, cnt;
};

__device__ __forceinline__ Window window_of(const ResampleArgs& a, int i) {
    Window w;
    const int64_t held = clamp_i64(a.len[i], 0, a.stride_in);
    w.in0 = a.in_start ? clamp_i64(a.in_start[i], 0, MAX_INDEX) : 0;
    w.o0 = a.out_start ? clamp_i64(a.out_start[i], 0, MAX_INDEX) : 0;
    const int64_t tot = a.total ? a.total[i] : held;
    w.n = w.in0 + held;
    const int64_t known = tot < 0 ? w.n : (tot > MAX_INDEX ? MAX_INDEX : tot);     // the length the outputs end at
    if (known < w.n) w.n = known;
    const int64_t lim = (known * a.p + a.q - 1) / a.q - w.o0;
    w.cnt = a.out_count ? clamp_i64(a.out_count[i], 0, a.stride_out) : a.stride_out;
    if (w.cnt > lim) w.cnt = lim < 0 ? 0 : lim;
    return w;
}

template <bool I16>
__global__ void __launch_bounds__(THREADS) resample_kernel(const ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* __restrict__ hs = smem;                     // [L]
    float* __restrict__ xs = (float*)(smem + a.L);      // [span]: xs[x] = x[kA + x]
    const int tid = threadIdx.x, i = a.sig_base + blockIdx.y;
    const Window w = window_of(a, i);
    const int64_t j0 = (int64_t)blockIdx.x * a.tile;
    const int64_t jstop = j0 + a.tile < a.stride_out ? j0 + a.tile : a.stride_out;    // the tile's part of the row
    float* __restrict__ out = a.out + (size_t)i * (size_t)a.stride_out;
    if (j0 >= w.cnt) {          // behind the last output: zeros, nothing staged
        for (int64_t j = j0 + tid; j < jstop; j += THREADS) out[j] = 0.f;
        return;
    }
    const int p = a.p, q = a.q, L = a.L, half = (L - 1) / 2;
    const int64_t jend = jstop < w.cnt ? jstop : w.cnt;
    // the samples the tile's outputs o0 + j0 .. o0 + jend - 1 meet, of those the row holds: [kA, kB]
    const int64_t loA = (int64_t)q * (w.o0 + j0) + half - (L - 1);
    int64_t kA = loA <= 0 ? 0 : (loA + p - 1) / p;
    if (kA < w.in0) kA = w.in0;
    int64_t kB = ((int64_t)q * (w.o0 + jend - 1) + half) / p;
    if (kB > w.n - 1) kB = w.n - 1;
    if (kB > kA + a.span - 1) kB = kA + a.span - 1;     // (never: resample_plan sized the span for the tile)
    const void* row = (const char*)a.in + (size_t)i * (size_t)a.stride_in * (I16 ? 2 : 4);
    for (int t = tid; t < L; t += THREADS) hs[t] = a.taps[t];
    const int staged = kB >= kA ? (int)(kB - kA + 1) : 0;       // at most span
    for (int x = tid; x < staged; x += THREADS) xs[x] = sample_at<I16>(row, kA + x - w.in0);
    __syncthreads();
    for (int64_t j = j0 + tid; j < jstop; j += THREADS) {
        float v = 0.f;
        if (j < jend) {
            const int64_t t0 = (int64_t)q * (w.o0 + j) + half, lo = t0 - (L - 1);
            int64_t k0 = lo <= 0 ? 0 : (lo + p - 1) / p, k1 = t0 / p;
            if (k0 < kA) k0 = kA;
            if (k1 > kB) k1 = kB;
            const int terms = k1 >= k0 ? (int)(k1 - k0 + 1) : 0;
            const float* __restrict__ xp = xs + (k0 - kA);
            const double* __restrict__ hp = hs + (t0 - (int64_t)p * k0);      // in [0, L): k0 >= lo / p, k0 <= t0 / p
            double acc = 0.0;
#pragma unroll 4
            for (int c = 0; c < terms; ++c) acc = fma((double)xp[c], hp[-(int64_t)p * c], acc);
            v = (float)acc;
        }
        out[j] = v;
    }
}

// p == q == 1: output m is sample m
template <bool I16>
__global__ void __launch_bounds__(THREADS) resample_copy_kernel(const ResampleArgs a) {
    const int tid = threadIdx.x, i = a.sig_base + blockIdx.y;
    const Window w = window_of(a, i);
    const int64_t j0 = (int64_t)blockIdx.x * a.tile;
    const int64_t jstop = j0 + a.tile < a.stride_out ? j0 + a.tile : a.stride_out;
    float* __restrict__ out = a.out + (size_t)i * (size_t)a.stride_out;
    const void* row = (const char*)a.in + (size_t)i * (size_t)a.stride_in * (I16 ? 2 : 4);
    for (int64_t j = j0 + tid; j < jstop; j += THREADS) {
        const int64_t k = w.o0 + j;
        out[j] = j < w.cnt && k >= w.in0 && k < w.n ? sample_at<I16>(row, k - w.in0) : 0.f;
    }
}

__global__ void __launch_bounds__(256) resample_taps_kernel(int p, int mpq, int L, double beta,
                                                            double* __restrict__ taps) {
    resample_taps_body(p, mpq, L, beta, taps);
}

// grid (ceil(stride_next / CARRY_BLOCK), n_sig)
template <typename T>
__global__ void __launch_bounds__(256)
resample_carry_kernel(const T* __restrict__ prev, int64_t stride_prev, const T* __restrict__ chunk,
                      int64_t stride_chunk, const int64_t* __restrict__ drop_, const int64_t* __restrict__ keep_,
                      const int64_t* __restrict__ add_, T* __restrict__ next, int64_t stride_next) {
    const int i = blockIdx.y;
    const int64_t drop = clamp_i64(drop_[i], 0, stride_prev);
    const int64_t room_p = stride_prev - drop;
    const int64_t keep = clamp_i64(keep_[i], 0, room_p < stride_next ? room_p : stride_next);
    const int64_t room_n = stride_next - keep;
    const int64_t add = clamp_i64(add_[i], 0, stride_chunk < room_n ? stride_chunk : room_n);
    const T* __restrict__ pr = prev + (size_t)i * (size_t)stride_prev + drop;
    const T* __restrict__ ch = chunk + (size_t)i * (size_t)stride_chunk;
    T* __restrict__ nx = next + (size_t)i * (size_t)stride_next;
    const int64_t j0 = (int64_t)blockIdx.x * CARRY_BLOCK;
    const int64_t jstop = j0 + CARRY_BLOCK < keep + add ? j0 + CARRY_BLOCK : keep + add;
    for (int64_t j = j0 + threadIdx.x; j < jstop; j += 256) nx[j] = j < keep ? pr[j] : ch[j - keep];
}

// once per kernel instance and device: the dynamic-LDS limit of the widest launch (as snmf_tile.h's launch_grid)
template <bool I16>
hipError_t raise_lds_limit(int device) {
    static std::atomic<bool> raised[64];
    if (device >= 0 && device < 64 && raised[device].load(std::memory_order_acquire)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void*)resample_kernel<I16>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
    if (e == hipSuccess && device >= 0 && device < 64) raised[device].store(true, std::memory_order_release);
    return e;
}

int32_t resample_launch(drnmf_handle_t h, const char* what, int32_t n_sig, int64_t stride_in, const int64_t* len,
                        const int64_t* in_start, const int64_t* out_start, const int64_t* out_count,
                        const int64_t* total, int32_t is_int16, const void* in, int32_t p, int32_t q, int32_t nz,
                        const double* taps, int64_t stride_out, float* out, hipStream_t stream) {
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (n_sig < 1 || stride_in < 1 || stride_in > MAX_STRIDE || stride_out < 1 || stride_out > MAX_STRIDE ||
        (is_int16 != 0 && is_int16 != 1))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: bad shape n_sig=%d stride_in=%lld stride_out=%lld is_int16=%d", what,
                   n_sig, (long long)stride_in, (long long)stride_out, is_int16);
    Plan pl;
    const bool copy = p == 1 && q == 1;
    if (!resample_plan(p, q, nz, &pl) || gcd_i64(p, q) != 1)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG,
                   "%s: p / q = %d / %d must be reduced with max(p, q) <= %d, and nz = %d a filter that fits in LDS",
                   what, p, q, MAX_PQ, nz);
    if (!len || !in || !out || (!copy && !taps)) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: NULL pointer argument", what);
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "%s: the handle is bound to no device", what);
    const int tile = copy ? TILE : pl.tile;
    const int64_t tiles = (stride_out + tile - 1) / tile;
    if (tiles > 0x7fffffff)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: stride_out=%lld is more than 2^31 - 1 tiles of %d outputs", what,
                   (long long)stride_out, tile);
    if (!copy) DRNMF_HIP(h, is_int16 ? raise_lds_limit<true>(h->device) : raise_lds_limit<false>(h->device));
    ResampleArgs a = {in, taps, len, in_start, out_start, out_count, total, out, stride_in, stride_out,
                      p, q, pl.L, tile, pl.span, 0};
    const size_t lds = copy ? 0 : pl.lds;
    const int max_y = 65535;        // rows on grid.y in slices, as mix.hip's launches
    for (int r0 = 0; r0 < n_sig; r0 += max_y) {
        a.sig_base = r0;
        const dim3 grid((unsigned)tiles, (unsigned)(n_sig - r0 < max_y ? n_sig - r0 : max_y));
        if (copy && is_int16)
            hipLaunchKernelGGL(resample_copy_kernel<true>, grid, dim3(THREADS), lds, stream, a);
        else if (copy)
            hipLaunchKernelGGL(resample_copy_kernel<false>, grid, dim3(THREADS), lds, stream, a);
        else if (is_int16)
            hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(THREADS), lds, stream, a);
        else
            hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(THREADS), lds, stream, a);
    }
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

}  // namespace

extern "C" int32_t drnmf_resample_rate(int64_t fs_in, int64_t fs_out, int32_t* p, int32_t* q) {
    if (fs_in <= 0 || fs_out <= 0 || !p || !q) return DRNMF_ERR_INVALID_ARG;
    const int64_t g = gcd_i64(fs_out, fs_in);
    const int64_t pp = fs_out / g, qq = fs_in / g;
    if (pp > MAX_PQ || qq > MAX_PQ) return DRNMF_ERR_INVALID_ARG;
    *p = (int32_t)pp;
    *q = (int32_t)qq;
    return DRNMF_OK;
}

extern "C" int64_t drnmf_resample_taps_len(int32_t p, int32_t q, int32_t nz) {
    Plan pl;
    if (!resample_plan(p, q, nz, &pl) || (p == 1 && q == 1)) return 0;
    return pl.L;
}

extern "C" int64_t drnmf_resample_out_len(int64_t n, int32_t p, int32_t q) {
    if (n < 0 || n > MAX_STRIDE || p < 1 || q < 1 || p > MAX_PQ || q > MAX_PQ) return 0;
    return (n * p + q - 1) / q;
}

extern "C" int32_t drnmf_resample_tile(int32_t p, int32_t q, int32_t nz) {
    Plan pl;
    if (!resample_plan(p, q, nz, &pl)) return 0;
    return p == 1 && q == 1 ? TILE : pl.tile;
}

extern "C" int32_t drnmf_resample_taps(drnmf_handle_t h, int32_t p, int32_t q, int32_t nz, double beta, double* taps,
                                       void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    Plan pl;
    if (!resample_plan(p, q, nz, &pl) || gcd_i64(p, q) != 1 || (p == 1 && q == 1) || !(beta >= 0.0) || !(beta < 1e3))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG,
                   "resample_taps: p / q = %d / %d must be reduced, not 1 / 1, with max(p, q) <= %d; nz = %d a filter "
                   "that fits in LDS; beta = %g in [0, 1000)", p, q, MAX_PQ, nz, beta);
    if (!taps) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "resample_taps: NULL pointer argument");
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "resample_taps: the handle is bound to no device");
    hipLaunchKernelGGL(resample_taps_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream_, p, p > q ? p : q, pl.L, beta,
                       taps);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

extern "C" int32_t drnmf_resample_forward(drnmf_handle_t h, int32_t n_sig, int64_t stride_in, const int64_t* len,
                                          int32_t is_int16, const void* in, int32_t p, int32_t q, int32_t nz,
                                          const double* taps, int64_t stride_out, float* out, void* stream_) {
    DRNMF_LOCK(h);
    return resample_launch(h, "resample_forward", n_sig, stride_in, len, nullptr, nullptr, nullptr, nullptr, is_int16,
                           in, p, q, nz, taps, stride_out, out, (hipStream_t)stream_);
}

extern "C" int32_t drnmf_resample_chunk(drnmf_handle_t h, int32_t n_sig, int64_t stride_in, const int64_t* len,
                                        const int64_t* in_start, const int64_t* out_start, const int64_t* out_count,
                                        const int64_t* total, int32_t is_int16, const void* in, int32_t p, int32_t q,
                                        int32_t nz, const double* taps, int64_t stride_out, float* out,
                                        void* stream_) {
    DRNMF_LOCK(h);
    return resample_launch(h, "resample_chunk", n_sig, stride_in, len, in_start, out_start, out_count, total, is_int16,
                           in, p, q, nz, taps, stride_out, out, (hipStream_t)stream_);
}

extern "C" int32_t drnmf_resample_carry(drnmf_handle_t h, int32_t n_sig, int32_t is_int16, int64_t stride_prev,
                                        const void* prev, int64_t stride_chunk, const void* chunk,
                                        const int64_t* drop, const int64_t* keep, const int64_t* add,
                                        int64_t stride_next, void* next, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (n_sig < 1 || n_sig > 65535 || stride_prev < 1 || stride_prev > MAX_STRIDE || stride_chunk < 0 ||
        stride_chunk > MAX_STRIDE || stride_next < 1 || stride_next > MAX_STRIDE || (is_int16 != 0 && is_int16 != 1))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG,
                   "resample_carry: bad shape n_sig=%d (at most 65535) is_int16=%d stride_prev=%lld stride_chunk=%lld "
                   "stride_next=%lld", n_sig, is_int16, (long long)stride_prev, (long long)stride_chunk,
                   (long long)stride_next);
    if (!prev || (!chunk && stride_chunk > 0) || !drop || !keep || !add || !next)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "resample_carry: NULL pointer argument");
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "resample_carry: the handle is bound to no device");
    const int64_t blocks = (stride_next + CARRY_BLOCK - 1) / CARRY_BLOCK;
    if (blocks > 0x7fffffff) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "resample_carry: stride_next too large");
    const dim3 grid((unsigned)blocks, (unsigned)n_sig);
    hipStream_t stream = (hipStream_t)stream_;
    if (is_int16)
        hipLaunchKernelGGL(resample_carry_kernel<short>, grid, dim3(256), 0, stream, (const short*)prev, stride_prev,
                           (const short*)chunk, stride_chunk, drop, keep, add, (short*)next, stride_next);
    else
        hipLaunchKernelGGL(resample_carry_kernel<float>, grid, dim3(256), 0, stream, (const float*)prev, stride_prev,
                           (const float*)chunk, stride_chunk, drop, keep, add, (float*)next, stride_next);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}
