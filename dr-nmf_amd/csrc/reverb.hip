// Device-side reverberator (include/drnmf_reverb.h): every signal of a speech bank convolved with one RIR of a bank,
// wet = early + late with the early part kept apart on request.  Direct-form convolution on the VALU: per output a
// single ascending chain of fmaf, which is what the header defines and what makes a signal's bits independent of
// its batch.  8192 taps per output are 8192 FMAs against 4 bytes written: compute bound by three orders.
//
// A workgroup of 256 threads owns one tile of 2048 outputs of one signal (grid.x: tiles, grid.y: signals in slices
// of at most 65535); thread p holds the 8 consecutive outputs 8 p .. 8 p + 7 of the tile in registers.  The taps
// are walked in chunks of 1024 counted from tap 0.  Per chunk the workgroup stages the chunk of h and the window
// of tile + chunk samples it meets in LDS (each sample read once from global memory, int16 converted there,
// zeros outside the signal), then every thread slides over the taps in groups of 8: 8 taps (two broadcast 16-byte
// reads) and the 16 samples around its outputs feed 64 FMAs; the lower 8 of those samples are the next group's
// upper 8 and stay in registers, so a group reads 8 new samples (two 16-byte reads): 16 dwords of LDS for 64 FMAs.
//
// LDS banks.  A lane's sample reads start 8 dwords after its neighbour's, so in a ds_read_b128 lane group (16
// lanes, whose lane numbers cover every residue mod 16; bank = dword mod 64, a 16-byte slot = 4 banks) lanes l and
// l + 8 would meet on one slot: two-way.  The window is therefore stored with neighbouring slots swapped inside every
// odd block of 64 dwords (x ^ 4 where bit 6 of x is set): slot(l) = (2 l + (l >> 3 & 1)) mod 16 is a bijection on
// residues mod 16, for every tap group.  The staging stores stay conflict-free (32 consecutive dwords permuted
// inside their 128 bytes).
//
// "Skipped" is exact, not "multiplied by zero": a group of 8 taps whose samples all lie inside the signal and
// whose taps all lie inside the part being summed runs unpredicated; any other group runs a predicated body that
// leaves the accumulator alone for a term outside (a non-finite tap or sample never reaches an output the
// definition keeps it from).
#include "common.h"
#include "../../include/drnmf_reverb.h"

namespace {

constexpr int TILE = DRNMF_REVERB_TILE;       // outputs per workgroup
constexpr int CHUNK = DRNMF_REVERB_CHUNK;     // taps staged at a time
constexpr int THREADS = 256;
constexpr int R = TILE / THREADS;             // consecutive outputs per thread
constexpr int WIN = TILE + CHUNK;             // staged samples: win[x] = s[k0 + d - t0 - CHUNK + x]
constexpr int64_t MAX_STRIDE_S = (int64_t)1 << 40;
constexpr int64_t MAX_STRIDE_R = (int64_t)1 << 30;
static_assert(R == 8, "a thread's outputs and a tap group are 8 wide: two 16-byte pieces each");
static_assert(CHUNK % 8 == 0 && WIN % 64 == 0, "whole tap groups, whole swizzle blocks");

__device__ __forceinline__ int64_t clamp_len(int64_t n, int64_t stride) {
    return n < 0 ? 0 : (n > stride ? stride : n);
}

template <bool I16>
__device__ __forceinline__ float sample_at(const void* __restrict__ row, int64_t m) {
    if constexpr (I16)
        return (float)((const short*)row)[m] / 32768.0f;      // as mix.hip and stft.hip read int16
    else
        return ((const float*)row)[m];
}

__device__ __forceinline__ int swz(int x) { return x ^ ((x >> 4) & 4); }    // bit 6 of x -> bit 2

struct ReverbArgs {
    const void* speech;
    const float* rirs;
    const int64_t* len_s;
    const int64_t* len_r;
    const int32_t* rir_index;
    const int32_t* delay;       // or NULL
    const int32_t* n_early;     // or NULL
    float* wet;
    float* early;               // or NULL
    int64_t stride_s, stride_r;
    int n_rir, sig_base;
    int vec_o;                  // the output rows take aligned quads
};

// One group of 8 taps h8 against the thread's window: a = win[base - 8 .. base - 1], b = win[base .. base + 7];
// output r meets tap v at win[base + r - v].  CHECK: a term counts only if its tap lies in [ua, ub) (u0: the
// group's first tap, chunk-local) and its window position in [lo, hi).
template <bool CHECK>
__device__ __forceinline__ void tap_group(float (&acc)[R], const float (&a)[8], const float (&b)[8],
                                          const float (&h8)[8], int base, int u0, int ua, int ub, int lo, int hi) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float s = r - v >= 0 ? b[r - v >= 0 ? r - v : 0] : a[r - v < 0 ? 8 + r - v : 0];
            if constexpr (CHECK) {
                const int x = base + r - v, u = u0 + v;
                const bool ok = u >= ua && u < ub && x >= lo && x < hi;
                acc[r] = ok ? fmaf(h8[v], s, acc[r]) : acc[r];
            } else {
                acc[r] = fmaf(h8[v], s, acc[r]);
            }
        }
    }
}

template <bool I16>
__global__ void __launch_bounds__(THREADS) reverb_forward_kernel(const ReverbArgs a) {
    __shared__ __attribute__((aligned(16))) float win[WIN];
    __shared__ __attribute__((aligned(16))) float hs[CHUNK];
    const int tid = threadIdx.x, i = a.sig_base + blockIdx.y, o0 = R * tid;
    const int64_t n = clamp_len(a.len_s[i], a.stride_s), k0 = (int64_t)blockIdx.x * TILE;
    const void* row = (const char*)a.speech + (size_t)i * (size_t)a.stride_s * (I16 ? 2 : 4);
    const int j = a.rir_index[i];
    const int L = j >= 0 && j < a.n_rir ? (int)clamp_len(a.len_r[j], a.stride_r) : 0;

    float acc[R], ev[R], wv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;

    if (L == 0 || k0 >= n) {
        // no RIR: the speech itself; behind the signal: zeros (the stores below)
        if (L == 0)
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (k0 + o0 + r < n) acc[r] = sample_at<I16>(row, k0 + o0 + r);
#pragma unroll
        for (int r = 0; r < R; ++r) ev[r] = wv[r] = acc[r];
    } else {
        int d = a.delay ? a.delay[j] : 0;
        d = d < 0 ? 0 : (d > L - 1 ? L - 1 : d);
        int E = a.n_early ? a.n_early[j] : L;
        E = E < 0 ? 0 : (E > L ? L : E);
        const float* __restrict__ h = a.rirs + (size_t)j * (size_t)a.stride_r;
        // the taps that can meet a sample of the signal from an output of this tile: t in [tlo, thi]
        const int64_t kend = k0 + TILE < n ? k0 + TILE : n;
        const int64_t tlo64 = k0 + d - (n - 1), thi64 = kend - 1 + d;
        const int tlo = tlo64 < 0 ? 0 : (tlo64 > L ? L : (int)tlo64);
        const int thi = thi64 > L - 1 ? L - 1 : (int)thi64;

        for (int phase = 0; phase < 2; ++phase) {
            // phase 0: the early taps [0, E); phase 1: the late taps [E, L)
            const int pa = phase ? E : 0, pb = phase ? L : E;
            const int ta = pa > tlo ? pa : tlo, tb = pb < thi + 1 ? pb : thi + 1;
            if (ta < tb) {
                for (int t0 = ta / CHUNK * CHUNK; t0 < tb; t0 += CHUNK) {
                    const int64_t wbase = k0 + d - t0 - CHUNK;
                    __syncthreads();        // the readers of the chunk before
                    for (int x = tid; x < WIN; x += THREADS) {
                        const int64_t m = wbase + x;
                        win[swz(x)] = m >= 0 && m < n ? sample_at<I16>(row, m) : 0.f;
                    }
                    for (int u = tid; u < CHUNK; u += THREADS) hs[u] = t0 + u < L ? h[t0 + u] : 0.f;
                    __syncthreads();
                    // window positions inside the signal: [lo, hi); taps of this part inside the chunk: [ua, ub)
                    const int lo = wbase >= 0 ? 0 : (-wbase > WIN ? WIN : (int)-wbase);
                    const int64_t hi64 = n - wbase;
                    const int hi = hi64 > WIN ? WIN : (hi64 < 0 ? 0 : (int)hi64);
                    const int ua = ta > t0 ? ta - t0 : 0, ub = tb - t0 < CHUNK ? tb - t0 : CHUNK;
                    // the lower 8 samples of one group are the upper 8 of the next: two groups per trip, the
                    // two halves swapping roles, so that a group costs two sample reads and no moves
                    const auto load8 = [&](float (&w)[8], int x) {
                        *(f32x4*)&w[0] = *(const f32x4*)&win[swz(x)];
                        *(f32x4*)&w[4] = *(const f32x4*)&win[swz(x + 4)];
                    };
                    const auto group = [&](int g, const float (&wa)[8], const float (&wb)[8]) {
                        const int base = o0 + CHUNK - 8 * g;
                        float h8[8];
                        *(f32x4*)&h8[0] = *(const f32x4*)&hs[8 * g];
                        *(f32x4*)&h8[4] = *(const f32x4*)&hs[8 * g + 4];
                        const bool whole = 8 * g >= ua && 8 * g + 8 <= ub && base - 7 >= lo && base + 7 < hi;
                        if (whole)
                            tap_group<false>(acc, wa, wb, h8, base, 8 * g, ua, ub, lo, hi);
                        else
                            tap_group<true>(acc, wa, wb, h8, base, 8 * g, ua, ub, lo, hi);
                    };
                    int g = ua / 8;
                    const int g_end = (ub + 7) / 8;
                    float w0[8], w1[8];
                    load8(w0, o0 + CHUNK - 8 * g);
                    for (; g + 1 < g_end; g += 2) {
                        load8(w1, o0 + CHUNK - 8 * g - 8);
                        group(g, w1, w0);
                        load8(w0, o0 + CHUNK - 8 * g - 16);
                        group(g + 1, w0, w1);
                    }
                    if (g < g_end) {
                        load8(w1, o0 + CHUNK - 8 * g - 8);
                        group(g, w1, w0);
                    }
                }
            }
            if (phase == 0) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    ev[r] = acc[r];
                    if (E < L) acc[r] = 0.f;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) wv[r] = E < L ? ev[r] + acc[r] : ev[r];
    }

    // every element of the tile's part of both rows; zeros from n on
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const bool in = k0 + o0 + r < n;
        wv[r] = in ? wv[r] : 0.f;
        ev[r] = in ? ev[r] : 0.f;
    }
    float* outs[2] = {a.wet, a.early};
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        if (!outs[w]) continue;
        float* out = outs[w] + (size_t)i * (size_t)a.stride_s;
        const float* v = w ? ev : wv;
#pragma unroll
        for (int q = 0; q < R; q += 4) {
            const int64_t k = k0 + o0 + q;
            if (a.vec_o) {
                if (k < a.stride_s) *(f32x4*)(out + k) = f32x4{v[q], v[q + 1], v[q + 2], v[q + 3]};   // stride_s % 4 == 0
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k + e < a.stride_s) out[k + e] = v[q + e];
            }
        }
    }
}

static bool aligned_rows(const void* p, int64_t stride) { return stride % 4 == 0 && ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int32_t drnmf_reverb_forward(drnmf_handle_t h, int32_t n_sig, int64_t stride_s, const int64_t* len_s,
                                        int32_t is_int16, const void* speech, int32_t n_rir, int64_t stride_r,
                                        const int64_t* len_r, const float* rirs, const int32_t* rir_index,
                                        const int32_t* delay, const int32_t* n_early, float* wet, float* early,
                                        void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (n_sig < 1 || stride_s < 1 || stride_s > MAX_STRIDE_S || n_rir < 1 || stride_r < 1 || stride_r > MAX_STRIDE_R ||
        (is_int16 != 0 && is_int16 != 1))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG,
                   "reverb_forward: bad shape n_sig=%d stride_s=%lld is_int16=%d n_rir=%d stride_r=%lld", n_sig,
                   (long long)stride_s, is_int16, n_rir, (long long)stride_r);
    if (!len_s || !speech || !len_r || !rirs || !rir_index || !wet)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "reverb_forward: NULL pointer argument");
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "reverb_forward: the handle is bound to no device");
    hipStream_t stream = (hipStream_t)stream_;
    ReverbArgs a = {speech, rirs, len_s, len_r, rir_index, delay, n_early, wet, early, stride_s, stride_r, n_rir, 0,
                    aligned_rows(wet, stride_s) && (!early || aligned_rows(early, stride_s)) ? 1 : 0};
    const unsigned tiles = (unsigned)((stride_s + TILE - 1) / TILE);
    const int max_y = 65535;        // rows on grid.y in slices, as mix.hip's launches
    for (int r0 = 0; r0 < n_sig; r0 += max_y) {
        a.sig_base = r0;
        const dim3 grid(tiles, (unsigned)(n_sig - r0 < max_y ? n_sig - r0 : max_y));
        if (is_int16)
            hipLaunchKernelGGL(reverb_forward_kernel<true>, grid, dim3(THREADS), 0, stream, a);
        else
            hipLaunchKernelGGL(reverb_forward_kernel<false>, grid, dim3(THREADS), 0, stream, a);
    }
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}
