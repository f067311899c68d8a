// Device-side mixer (include/drnmf_mix.h): noisy = speech + g * noise at a requested SNR, from a speech bank and a
// noise bank that stay in HBM.  Two passes over the samples (the noise segment's energy, then the mix) around one
// small launch that turns the block partial sums into the gains; a third pass (the speech energy) only when the
// caller did not keep it.  Memory bound: per sample 4 bytes of speech, the noise read twice, 4 bytes written.
//
// A workgroup of 256 threads owns one block of 4096 samples of one signal (grid.x: blocks, grid.y: signals in
// slices of at most 65535).  Thread t takes the four quads at 1024 c + 4 t, c = 0..3, so that a wave's accesses on
// the speech and output side are contiguous 16-byte pieces; the noise side starts at an arbitrary offset and is
// read with 4-byte (float32) or 2-byte (int16) alignment.  The position in the noise recording is reduced modulo
// its length once per thread (the only 64-bit divisions; a 32-bit fast path measured no faster), then advanced by
// compare-and-subtract.
//
// Every sum has a fixed order (drnmf_mix.h) and nothing is shared between workgroups but the partial sums one
// launch writes and the next reads: no atomics, no waiting, the same bits at any batch position.
#include "common.h"
#include "../../include/drnmf_mix.h"

namespace {

constexpr int BLOCK = DRNMF_MIX_BLOCK;        // samples per workgroup
constexpr int QUADS = 4;                      // quads of four samples per thread
constexpr int QSTEP = BLOCK / QUADS;          // distance between a thread's quads
constexpr int64_t MAX_STRIDE = (int64_t)1 << 40;   // keeps offset + sample index far inside an int64
static_assert(QSTEP == 4 * 256, "256 threads x 4 samples per quad row");

typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte load at float alignment
struct alignas(2) s16x4_u { short v[4]; };                                // an 8-byte load at int16 alignment

__device__ __forceinline__ int64_t clamp_len(int64_t n, int64_t stride) {
    return n < 0 ? 0 : (n > stride ? stride : n);
}

__device__ __forceinline__ float pcm16(short v) { return (float)v / 32768.0f; }   // as stft.hip's frames read it

// Samples k .. k + 3 (k a multiple of 4) of a row of n samples; zeros behind n.  vec: the row's quads are
// 16-byte (float32) / 8-byte (int16) aligned.
template <bool I16>
__device__ __forceinline__ f32x4 own_quad(const void* __restrict__ row, int64_t k, int64_t n, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec && k + 3 < n) {
        if constexpr (I16) {
            const short4 r = *(const short4*)((const short*)row + k);
            v = f32x4{pcm16(r.x), pcm16(r.y), pcm16(r.z), pcm16(r.w)};
        } else {
            v = *(const f32x4*)((const float*)row + k);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < n) v[e] = I16 ? pcm16(((const short*)row)[k + e]) : ((const float*)row)[k + e];
    }
    return v;
}

// Where a thread stands in its signal's noise recording: row of L >= 1 samples, position p in [0, L), and the
// step between two of the thread's quads, already reduced.
struct Seg {
    const void* row;
    int64_t L, p, step;
};

struct MixArgs {
    const void* speech;
    const void* noise;
    const int64_t* len_s;
    const int64_t* len_n;
    const int32_t* noise_index;
    const int64_t* offset;
    int64_t stride_s, stride_n;
    double* partial_n;      // [n_sig][nblk]: the segment-energy partial sums
    const float* g;         // [n_sig]
    float* noisy;           // [n_sig][stride_s]
    int64_t nblk;
    int n_sig, n_noise, sig_base;
    int vec_s, vec_o;       // the speech / the output rows take aligned quads
};

// false: signal i has no noise to read (index out of range, empty recording)
template <bool NI16>
__device__ __forceinline__ bool seg_open(const MixArgs& a, int i, int64_t k, Seg& s) {
    const int j = a.noise_index[i];
    if (j < 0 || j >= a.n_noise) return false;
    const int64_t L = clamp_len(a.len_n[j], a.stride_n);
    if (L == 0) return false;
    int64_t o = a.offset[i] % L;
    if (o < 0) o += L;
    s.row = (const char*)a.noise + (size_t)j * (size_t)a.stride_n * (NI16 ? 2 : 4);
    s.L = L;
    s.p = (o + k) % L;
    s.step = QSTEP % L;
    return true;
}

// noise at positions p, p + 1, p + 2, p + 3, wrapped (L may be shorter than the quad)
template <bool NI16>
__device__ __forceinline__ f32x4 seg_quad(const Seg& s) {
    f32x4 v;
    if (s.p + 3 < s.L) {
        if constexpr (NI16) {
            s16x4_u r;
            __builtin_memcpy(&r, (const short*)s.row + s.p, sizeof(r));
            v = f32x4{pcm16(r.v[0]), pcm16(r.v[1]), pcm16(r.v[2]), pcm16(r.v[3])};
        } else {
            v = *(const f32x4_u*)((const float*)s.row + s.p);
        }
    } else {
        int64_t q = s.p;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = NI16 ? pcm16(((const short*)s.row)[q]) : ((const float*)s.row)[q];
            q = q + 1 == s.L ? 0 : q + 1;
        }
    }
    return v;
}

__device__ __forceinline__ void seg_advance(Seg& s) {
    s.p += s.step;
    if (s.p >= s.L) s.p -= s.L;
}

// The workgroup's sum of `acc`, in every thread of wave 0 .. 3 alike: a butterfly inside each wave (both partners
// add the same pair), then the four waves in wave order.
__device__ __forceinline__ double block_sum(double acc, double* red, int tid) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ double sumsq(double acc, const f32x4 v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc += (double)v[e] * (double)v[e];       // the product is exact
    return acc;
}

struct EnergyArgs {
    const void* pcm;
    const int64_t* len;
    int64_t stride;
    double* partial;        // [n_sig][nblk]
    int64_t nblk;
    int sig_base, vec;
};

// partial[i][b] = the sum of squares of block b of signal i; blocks behind the signal's length write nothing
template <bool I16>
__global__ void __launch_bounds__(256) mix_energy_kernel(const EnergyArgs a) {
    __shared__ double red[4];
    const int tid = threadIdx.x, i = a.sig_base + blockIdx.y;
    const int64_t n = clamp_len(a.len[i], a.stride), k0 = (int64_t)blockIdx.x * BLOCK;
    if (k0 >= n) return;
    const void* row = (const char*)a.pcm + (size_t)i * (size_t)a.stride * (I16 ? 2 : 4);
    f32x4 v[QUADS];
#pragma unroll
    for (int c = 0; c < QUADS; ++c) v[c] = own_quad<I16>(row, k0 + c * QSTEP + 4 * tid, n, a.vec != 0);
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < QUADS; ++c) acc = sumsq(acc, v[c]);
    acc = block_sum(acc, red, tid);
    if (tid == 0) a.partial[(size_t)i * a.nblk + blockIdx.x] = acc;
}

// partial_n[i][b] = the sum of squares of the noise segment under block b of signal i
template <bool NI16>
__global__ void __launch_bounds__(256) mix_segment_energy_kernel(const MixArgs a) {
    __shared__ double red[4];
    const int tid = threadIdx.x, i = a.sig_base + blockIdx.y;
    const int64_t n = clamp_len(a.len_s[i], a.stride_s), k0 = (int64_t)blockIdx.x * BLOCK;
    if (k0 >= n) return;
    Seg s;
    if (!seg_open<NI16>(a, i, k0 + 4 * tid, s)) return;
    // every load of the thread first, then the sum in its order
    f32x4 v[QUADS];
#pragma unroll
    for (int c = 0; c < QUADS; ++c) {
        const int64_t k = k0 + c * QSTEP + 4 * tid;
        v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (k < n) v[c] = seg_quad<NI16>(s);
        seg_advance(s);
    }
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < QUADS; ++c) {
        const int64_t k = k0 + c * QSTEP + 4 * tid;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[c][e] = k + e < n ? v[c][e] : 0.f;
        acc = sumsq(acc, v[c]);
    }
    acc = block_sum(acc, red, tid);
    if (tid == 0) a.partial_n[(size_t)i * a.nblk + blockIdx.x] = acc;
}

// noisy[i][k] for the block's k < stride_s
template <bool SI16, bool NI16>
__global__ void __launch_bounds__(256) mix_apply_kernel(const MixArgs a) {
    const int tid = threadIdx.x, i = a.sig_base + blockIdx.y;
    const int64_t n = clamp_len(a.len_s[i], a.stride_s), k0 = (int64_t)blockIdx.x * BLOCK;
    const void* row = (const char*)a.speech + (size_t)i * (size_t)a.stride_s * (SI16 ? 2 : 4);
    float* out = a.noisy + (size_t)i * (size_t)a.stride_s;
    const float g = a.g[i];
    Seg s;
    // g != 0 only for a signal whose noise exists (mix_gain_kernel)
    const bool mixing = g != 0.f && k0 < n && seg_open<NI16>(a, i, k0 + 4 * tid, s);
    // every load of the thread first (speech, then noise), then the arithmetic and the stores
    f32x4 v[QUADS], z[QUADS];
#pragma unroll
    for (int c = 0; c < QUADS; ++c) {
        const int64_t k = k0 + c * QSTEP + 4 * tid;
        v[c] = own_quad<SI16>(row, k, n, a.vec_s != 0);       // zeros from n on
    }
    if (mixing) {
#pragma unroll
        for (int c = 0; c < QUADS; ++c) {
            const int64_t k = k0 + c * QSTEP + 4 * tid;
            z[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (k < n) z[c] = seg_quad<NI16>(s);
            seg_advance(s);
        }
#pragma unroll
        for (int c = 0; c < QUADS; ++c) {
            const int64_t k = k0 + c * QSTEP + 4 * tid;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[c][e] = k + e < n ? fmaf(g, z[c][e], v[c][e]) : 0.f;
        }
    }
#pragma unroll
    for (int c = 0; c < QUADS; ++c) {
        const int64_t k = k0 + c * QSTEP + 4 * tid;
        if (a.vec_o) {
            if (k < a.stride_s) *(f32x4*)(out + k) = v[c];    // stride_s is a multiple of 4: the quad is inside the row
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (k + e < a.stride_s) out[k + e] = v[c][e];
        }
    }
}

// sum_{b < nb} p[b] in ascending order with eight loads in flight (common.h's ordered_sum in fp64)
__device__ __forceinline__ double sum_blocks(const double* __restrict__ p, int64_t nb) {
    double acc = 0.0;
    for (int64_t b0 = 0; b0 < nb; b0 += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[b0 + u < nb ? b0 + u : nb - 1];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += b0 + u < nb ? v[u] : 0.0;
    }
    return acc;
}

__device__ __forceinline__ int64_t blocks_of(int64_t n) { return (n + BLOCK - 1) / BLOCK; }

// energy[i] = the blocks' partial sums in ascending order; one lane per signal
__global__ void __launch_bounds__(64) mix_energy_sum_kernel(const double* __restrict__ partial,
                                                            const int64_t* __restrict__ len, int64_t stride,
                                                            int64_t nblk, int n_sig, double* __restrict__ energy) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_sig) return;
    energy[i] = sum_blocks(partial + (size_t)i * nblk, blocks_of(clamp_len(len[i], stride)));
}

struct GainArgs {
    const double* partial_n;
    const double* speech_energy;
    const int64_t* len_s;
    const int64_t* len_n;
    const int32_t* noise_index;
    const float* snr_db;
    float* g;               // [n_sig], the mix kernel's
    float* gain;            // [n_sig] of the caller, or NULL
    int64_t stride_s, stride_n, nblk;
    int n_sig, n_noise;
};

// g[i] of drnmf_mix.h; one lane per signal
__global__ void __launch_bounds__(64) mix_gain_kernel(const GainArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n_sig) return;
    const int j = a.noise_index[i];
    const float snr = a.snr_db[i];
    float g = 0.f;
    if (j >= 0 && j < a.n_noise && clamp_len(a.len_n[j], a.stride_n) > 0 && isfinite(snr)) {
        const double es = a.speech_energy[i];
        const double en = sum_blocks(a.partial_n + (size_t)i * a.nblk, blocks_of(clamp_len(a.len_s[i], a.stride_s)));
        if (es != 0.0 && en != 0.0) {
            const float gf = (float)(sqrt(es / en) * pow(10.0, (double)snr * -0.05));
            if (isfinite(gf)) g = gf;
        }
    }
    a.g[i] = g;
    if (a.gain) a.gain[i] = g;
}

// the workspace: both sets of partial sums, the speech energies, the gains
struct Layout {
    int64_t nblk;
    size_t off_partial_n, off_partial_s, off_energy, off_g, total;
};

static bool shape_ok(int32_t n_sig, int64_t stride) { return n_sig > 0 && stride > 0 && stride <= MAX_STRIDE; }

static Layout layout(int32_t n_sig, int64_t stride_s) {
    Layout l;
    l.nblk = (stride_s + BLOCK - 1) / BLOCK;
    const size_t part = (size_t)n_sig * (size_t)l.nblk * sizeof(double);
    l.off_partial_n = 0;
    l.off_partial_s = part;
    l.off_energy = 2 * part;
    l.off_g = l.off_energy + (size_t)n_sig * sizeof(double);
    l.total = round_up_sz(l.off_g + (size_t)n_sig * sizeof(float), 256);
    return l;
}

// rows on grid.y in slices of at most 65535, as stft.hip's pair launches
template <class F>
static void for_row_slices(int32_t n_sig, F&& f) {
    const int max_y = 65535;
    for (int r0 = 0; r0 < n_sig; r0 += max_y) f(r0, (unsigned)(n_sig - r0 < max_y ? n_sig - r0 : max_y));
}

static bool aligned_rows(const void* p, int64_t stride, size_t bytes) {
    return stride % 4 == 0 && ((uintptr_t)p & (bytes - 1)) == 0;
}

static void enqueue_energy(int32_t n_sig, int64_t stride, const int64_t* len, int32_t is_int16, const void* pcm,
                           double* partial, int64_t nblk, double* energy, hipStream_t stream) {
    EnergyArgs a = {pcm, len, stride, partial, nblk, 0, aligned_rows(pcm, stride, is_int16 ? 8 : 16) ? 1 : 0};
    for_row_slices(n_sig, [&](int r0, unsigned rows) {
        a.sig_base = r0;
        const dim3 grid((unsigned)nblk, rows);
        if (is_int16)
            hipLaunchKernelGGL(mix_energy_kernel<true>, grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL(mix_energy_kernel<false>, grid, dim3(256), 0, stream, a);
    });
    hipLaunchKernelGGL(mix_energy_sum_kernel, dim3((unsigned)((n_sig + 63) / 64)), dim3(64), 0, stream,
                       (const double*)partial, len, stride, nblk, n_sig, energy);
}

static int32_t check_workspace(drnmf_handle_t h, const char* who, const void* workspace, size_t have, size_t need) {
    if (!workspace || have < need)
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "%s: workspace %zu < required %zu", who, workspace ? have : (size_t)0,
                   need);
    return DRNMF_OK;
}

}  // namespace

extern "C" size_t drnmf_mix_workspace_bytes(int32_t n_sig, int64_t stride_s) {
    return shape_ok(n_sig, stride_s) ? layout(n_sig, stride_s).total : 0;
}

extern "C" int32_t drnmf_mix_energy(drnmf_handle_t h, int32_t n_sig, int64_t stride, const int64_t* len,
                                    int32_t is_int16, const void* pcm, double* energy, void* workspace,
                                    size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (!shape_ok(n_sig, stride) || (is_int16 != 0 && is_int16 != 1))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "mix_energy: bad shape n_sig=%d stride=%lld is_int16=%d", n_sig,
                   (long long)stride, is_int16);
    if (!len || !pcm || !energy) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "mix_energy: NULL pointer argument");
    const Layout l = layout(n_sig, stride);
    if (int32_t rc = check_workspace(h, "mix_energy", workspace, workspace_bytes, l.total)) return rc;
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "mix_energy: the handle is bound to no device");
    enqueue_energy(n_sig, stride, len, is_int16, pcm, (double*)((char*)workspace + l.off_partial_s), l.nblk, energy,
                   (hipStream_t)stream_);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

extern "C" int32_t drnmf_mix_forward(drnmf_handle_t h, int32_t n_sig, int64_t stride_s, const int64_t* len_s,
                                     int32_t s_is_int16, const void* speech, int32_t n_noise, int64_t stride_n,
                                     const int64_t* len_n, int32_t n_is_int16, const void* noise,
                                     const int32_t* noise_index, const int64_t* offset, const float* snr_db,
                                     const double* speech_energy, float* noisy, float* gain, void* workspace,
                                     size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (!shape_ok(n_sig, stride_s) || !shape_ok(n_noise, stride_n) || (s_is_int16 != 0 && s_is_int16 != 1) ||
        (n_is_int16 != 0 && n_is_int16 != 1))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG,
                   "mix_forward: bad shape n_sig=%d stride_s=%lld s_is_int16=%d n_noise=%d stride_n=%lld "
                   "n_is_int16=%d", n_sig, (long long)stride_s, s_is_int16, n_noise, (long long)stride_n,
                   n_is_int16);
    if (!len_s || !speech || !len_n || !noise || !noise_index || !offset || !snr_db || !noisy)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "mix_forward: NULL pointer argument");
    const Layout l = layout(n_sig, stride_s);
    if (int32_t rc = check_workspace(h, "mix_forward", workspace, workspace_bytes, l.total)) return rc;
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "mix_forward: the handle is bound to no device");
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    if (!speech_energy) {
        enqueue_energy(n_sig, stride_s, len_s, s_is_int16, speech, (double*)(ws + l.off_partial_s), l.nblk,
                       (double*)(ws + l.off_energy), stream);
        speech_energy = (const double*)(ws + l.off_energy);
    }
    MixArgs a = {speech, noise, len_s, len_n, noise_index, offset, stride_s, stride_n,
                 (double*)(ws + l.off_partial_n), (const float*)(ws + l.off_g), noisy, l.nblk, n_sig, n_noise, 0,
                 aligned_rows(speech, stride_s, s_is_int16 ? 8 : 16) ? 1 : 0, aligned_rows(noisy, stride_s, 16) ? 1 : 0};
    for_row_slices(n_sig, [&](int r0, unsigned rows) {
        a.sig_base = r0;
        const dim3 grid((unsigned)l.nblk, rows);
        if (n_is_int16)
            hipLaunchKernelGGL(mix_segment_energy_kernel<true>, grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL(mix_segment_energy_kernel<false>, grid, dim3(256), 0, stream, a);
    });
    const GainArgs ga = {a.partial_n, speech_energy, len_s, len_n, noise_index, snr_db, (float*)(ws + l.off_g), gain,
                         stride_s, stride_n, l.nblk, n_sig, n_noise};
    hipLaunchKernelGGL(mix_gain_kernel, dim3((unsigned)((n_sig + 63) / 64)), dim3(64), 0, stream, ga);
    for_row_slices(n_sig, [&](int r0, unsigned rows) {
        a.sig_base = r0;
        const dim3 grid((unsigned)l.nblk, rows);
        if (s_is_int16 && n_is_int16)
            hipLaunchKernelGGL((mix_apply_kernel<true, true>), grid, dim3(256), 0, stream, a);
        else if (s_is_int16)
            hipLaunchKernelGGL((mix_apply_kernel<true, false>), grid, dim3(256), 0, stream, a);
        else if (n_is_int16)
            hipLaunchKernelGGL((mix_apply_kernel<false, true>), grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL((mix_apply_kernel<false, false>), grid, dim3(256), 0, stream, a);
    });
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}
