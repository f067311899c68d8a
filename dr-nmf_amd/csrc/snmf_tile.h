// What the sparse-NMF tile kernels share, written once.  Every one of them gives a workgroup of four waves 16
// frame rows, keeps H in LDS, stages the dictionary 32 bins at a time through registers into LDS and runs the
// exact-fp32 MFMA.  Here: the slot map of the two products, the dictionary stager, the Masking pass and H's first
// value, the wave's partial of H Wc^T and the wave-order sum of the four, acc += A Wc, the numerator's chunk, the
// walk over a lane's own elements of H, the final-mask loop, the exit of a tile whose rows are all masked, the
// LDS size and the N limit, the launch with its dynamic-LDS limit, and the host's argument checks and instance
// choice.  What defines the baseline's result is written here once.  The users and what each may vary:
//
//   snmf_mask.hip   snmf_mask_tile_kernel: beta == 2.  Its own: the floor of Lambda and the update
//                   H num / max(den + sparsity, flr); it also keeps its initial loop, Lambda sum and update loop
//                   written out (init_h, lambda_sum and for_own_h say the same; measured slower there).
//   snmf_kl.hip     snmf_kl_tile_kernel: beta == 1.  The accumulators' roles (one float of den per column, num per
//                   iteration), the quotient V / Lambda in Lambda's slots, V's chunk in registers.
//   snmf_adapt.hip  snmf_adapt_h_kernel, snmf_adapt_stats_kernel, snmf_adapt_final_kernel: a dictionary per batch
//                   row (the stager's W), validity and H from global memory in place of the prologue, an LDS tail
//                   of their own (a V chunk buffer; the statistics' V / Lambda tiles).
//   snmf_online.hip snmf_online_h_kernel: snmf_mask_tile_kernel's loop on a dictionary per batch row, the row's block
//                   buffer as x and its to-do flags as validity, all through the functions here.
//   snmf_f16.hip    snmf_f16_tile_kernel: the row scale (rs: nullptr = none, and then no multiply either; else
//                   s[rl] multiplies V and the mask's epsilon), a stager of its own (a callable of final_mask; the
//                   fp32 dictionary is read twice in all) and fp16 iterations with their own maps and a wider
//                   stride of Lp; the fp32 phases in front of and behind them are the ones here.
//
// The per-wave partials in Lp are TR * LLD floats apart in every fp32 phase.
// Everything is passed as plain pointer and int arguments: no tile state is held across the kernel.
//
// Layout.  Hs [16][LD], Ws [32][LD], LD = Np + 8 (Np = N rounded up to 16).  LD % 16 == 8 makes both operand
// reads conflict-free: the 16-byte reads of the first product (lane (r, q) reads row r, atoms 16 S + 4 q ..)
// spread each 16-lane group of ds_read_b128 over all 64 banks, and the 4-byte reads of the second (lane (r, q)
// reads bin rows two apart for q and q + 1, see bin_base) put the two rows of a 32-lane group 16 banks apart.
// Lane l of wave w: r = l & 15, q = l >> 4; wave w owns the 16-atom blocks and the 16-column tiles w, w + 4, ..
#pragma once
#include "common.h"

#include <atomic>
#include <initializer_list>
#include <type_traits>

namespace snmf_tile {

constexpr int TR = 16;            // rows per workgroup (one MFMA M-tile)
constexpr int FC = 32;            // bins per staged dictionary chunk
constexpr int LLD = 36;           // row stride of the 16 x 32 partial / V chunk buffers
constexpr int MAX_N = 512;        // atoms a tile kernel takes (NTW = 8 tiles per wave)

constexpr int np16(int N) { return (N + 15) & ~15; }

// Dynamic LDS of a tile kernel: Hs [TR][LD], Ws [FC][LD], Lp [4][TR][lp_stride] and a tail (valid [TR]; a kernel
// with more behind Lp says how many floats)
constexpr size_t lds_bytes(int N, int lp_stride = LLD, int tail_floats = TR) {
    return ((size_t)(TR + FC) * (np16(N) + 8) + 4 * TR * lp_stride + tail_floats) * sizeof(float);
}
static_assert(lds_bytes(2) == 13888 && lds_bytes(200) == 50752 && lds_bytes(256) == 59968 &&
              lds_bytes(MAX_N) == 109120, "the tile kernels' LDS");

// Contraction slot (q, e) of the second product's k-step S' is bin 16 S' + bin_base(q) + (e & 1) + 4 (e >> 1):
// lanes q and q + 1 of one 32-lane group read dictionary rows two bins apart.
__device__ __forceinline__ int bin_base(int q) { return 8 * (q >> 1) + 2 * (q & 1); }

// V = x^power (enhance.py:838)
__device__ __forceinline__ float vpow(float xv, float power) {
    return power == 1.f ? xv : (power == 2.f ? xv * xv : powf(xv, power));
}

// v, or v s[rl] under a row scale
template <class RS>
__device__ __forceinline__ float row_scaled(float v, RS rs, int rl) {
    if constexpr (std::is_null_pointer_v<RS>) return v;
    else return v * rs[rl];
}

// A dictionary chunk on its way global -> registers (in flight under the previous chunk's products) -> LDS: wave w
// takes the chunk's rows w, w + 4, ..  VEC: N % 4 == 0 and W 16-byte aligned, 16-byte loads.  Ws is zero behind F
// and N.
template <int NTW, bool VEC>
struct Chunk {
    f32x4 v4[VEC ? FC / 4 : 1][VEC ? NTW / 4 : 1];
    float v1[VEC ? 1 : FC / 4][VEC ? 1 : NTW];
};

template <int NTW, bool VEC>
__device__ __forceinline__ void gload(Chunk<NTW, VEC>& p, const float* __restrict__ W, int c, int F, int N, int w,
                                      int l) {
    // (the row's offset below: bin and N are not negative, and said with the casts it is one 32 x 32 -> 64 bit
    // multiply; without them the compiler widens N outside the chunk loop and pays a 64 x 32 bit one per row in it)
#pragma unroll
    for (int i = 0; i < FC / 4; ++i) {
        const int bin = c * FC + w + 4 * i;
        if constexpr (VEC) {
#pragma unroll
            for (int k = 0; k < NTW / 4; ++k) {
                const int col = 4 * (l + 64 * k);
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (bin < F && col < N) v = *(const f32x4*)(W + (size_t)(unsigned)bin * (unsigned)N + col);
                p.v4[i][k] = v;
            }
        } else {
#pragma unroll
            for (int k = 0; k < NTW; ++k) {
                const int col = l + 64 * k;
                float v = 0.f;
                if (bin < F && col < N) v = W[(size_t)(unsigned)bin * (unsigned)N + col];
                p.v1[i][k] = v;
            }
        }
    }
}

template <int NTW, bool VEC>
__device__ __forceinline__ void swrite(const Chunk<NTW, VEC>& p, float* Ws, int LD, int Np, int w, int l) {
#pragma unroll
    for (int i = 0; i < FC / 4; ++i) {
        float* dst = Ws + (w + 4 * i) * LD;
        if constexpr (VEC) {
#pragma unroll
            for (int k = 0; k < NTW / 4; ++k) {
                const int col = 4 * (l + 64 * k);
                if (col < Np) *(f32x4*)(dst + col) = p.v4[i][k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < NTW; ++k) {
                const int col = l + 64 * k;
                if (col < Np) dst[col] = p.v1[i][k];
            }
        }
    }
}

// keras.layers.Masking: a frame is masked when every bin equals mask_value (lstm_pack_x_kernel's rule); a row behind
// `rows` is not valid.  Wave w decides the rows 4 w .. 4 w + 3.  A barrier belongs behind it.
__device__ __forceinline__ void row_validity(const float* x, int* valid, int64_t row0, int64_t rows, int F,
                                             float mask_value, int has_mask, int w, int l) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rl = 4 * w + i;
        const int64_t row = row0 + rl;
        bool any = false;
        if (row < rows) {
            if (has_mask) {
                for (int f = l; f < F; f += 64) any |= (x[row * F + f] != mask_value);
            } else {
                any = true;
            }
        }
        any = __any(any);
        if (l == 0) valid[rl] = any ? 1 : 0;
    }
}

// f(i, v, row, col) for this lane's own elements of H (and of num and den): element v of its tile i, which is
// row 4 q + v, column 16 t + r of the tile t = w + 4 i < NT
template <int NTW, class Fn>
__device__ __forceinline__ void for_own_h(int NT, int w, int r, int q, Fn&& f) {
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int t = w + 4 * i;
        if (t < NT) {
#pragma unroll
            for (int v = 0; v < 4; ++v) f(i, v, 4 * q + v, 16 * t + r);
        }
    }
}

// Hs = h_init on valid rows, 0 elsewhere and behind N, for exactly the columns of the tiles t < NT (for_own_h's
// elements.  Written out: with the select inside for_own_h's branch the compiler carries the tiles' t < NT
// conditions inverted through the chunk loop and pays a VALU compare for each)
template <int NTW>
__device__ __forceinline__ void init_h(float* Hs, const float* h_init, const int* valid, int N, int NT, int LD, int w,
                                       int r, int q) {
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int t = w + 4 * i, col = 16 * t + r;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int rl = 4 * q + v;
            float hv = 0.f;
            if (t < NT && col < N && valid[rl]) hv = h_init[col];
            if (t < NT) Hs[rl * LD + col] = hv;
        }
    }
}

// This wave's share of H Wc^T (its 16-atom blocks), 16 x 32, into its slot of Lp.  SEL 0: all atoms;
// 1: the atoms below rh only; 2: the atoms from rh on (the two halves of the mask).
template <int NTW, int SEL>
__device__ __forceinline__ void lambda_partial(const float* Hs, const float* Ws, float* Lp, int LD, int NT,
                                               int w, int r, int q, int rh) {
    f32x4 P[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int S = w + 4 * i;
        if (S < NT) {
            const int k0 = 16 * S + 4 * q;
            f32x4 a = *(const f32x4*)(Hs + r * LD + k0);
            if constexpr (SEL != 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] = ((k0 + e < rh) == (SEL == 1)) ? a[e] : 0.f;
            }
            const f32x4 b0 = *(const f32x4*)(Ws + r * LD + k0);
            const f32x4 b1 = *(const f32x4*)(Ws + (16 + r) * LD + k0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                P[0] = mfma16(a[e], b0[e], P[0]);
                P[1] = mfma16(a[e], b1[e], P[1]);
            }
        }
    }
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int v = 0; v < 4; ++v) Lp[(w * TR + 4 * q + v) * LLD + 16 * jt + r] = P[jt][v];
}

// The four waves' partials of Lambda_c added in wave order, ((p0 + p1) + p2) + p3, for this lane's operand slots of
// the second product: s[S'][e] is row r, bin 16 S' + bin_base(q) + (e & 1) + 4 (e >> 1)
__device__ __forceinline__ void lambda_sum(const float* Lp, int r, int q, float (&s)[2][4]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const float* p = Lp + r * LLD + 16 * ks + bin_base(q) + 4 * hh;
            f32x2 sum = *(const f32x2*)p;
            sum += *(const f32x2*)(p + TR * LLD);
            sum += *(const f32x2*)(p + 2 * TR * LLD);
            sum += *(const f32x2*)(p + 3 * TR * LLD);
            s[ks][2 * hh] = sum[0];
            s[ks][2 * hh + 1] = sum[1];
        }
}

// acc [16 x N] += A [16 x 32] Wc, A given as this lane's operand values aF[S'][e] (row r, bin slot (q, e))
template <int NTW>
__device__ __forceinline__ void accumulate(const float* Ws, int LD, int NT, int w, int r, int q,
                                           const float (&aF)[2][4], f32x4 (&acc)[NTW]) {
    const float* bq = Ws + bin_base(q) * LD + r;
#pragma unroll
    for (int i = 0; i < NTW; ++i) {           // (one wave-uniform branch per tile; another wave's MFMAs fill the
        const int t = w + 4 * i;              // dependent-accumulator latency of the chain of eight)
        if (t < NT) {
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    acc[i] = mfma16(aF[s][e], bq[(16 * s + (e & 1) + 4 * (e >> 1)) * LD + 16 * t], acc[i]);
        }
    }
}

// The numerator's chunk c, first half: V = x^power (times the row's scale) on valid rows, 0 elsewhere and behind
// F, into slot 0 of Lp.  A barrier belongs between the two halves.
template <class RS>
__device__ __forceinline__ void num_fill(const float* x, float* Lp, const int* valid, RS rs, int64_t row0, int F,
                                         int c, float power, int tid) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int idx = tid + 256 * k, rl = idx >> 5, b = idx & 31, f = c * FC + b;
        float v = 0.f;
        if (valid[rl] && f < F) v = row_scaled(vpow(x[(row0 + rl) * F + f], power), rs, rl);
        Lp[rl * LLD + b] = v;
    }
}
// ... second half: num += V_c Wc
template <int NTW>
__device__ __forceinline__ void num_accumulate(const float* Ws, const float* Lp, int LD, int NT, int w, int r, int q,
                                               f32x4 (&num)[NTW]) {
    float aF[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) aF[s][e] = Lp[r * LLD + 16 * s + bin_base(q) + (e & 1) + 4 * (e >> 1)];
    accumulate<NTW>(Ws, LD, NT, w, r, q, aF, num);
}

// mask = Wc Hc / (s 1e-9 + Wc Hc + Wn Hn) from the fp32 H in Hs, a chunk at a time (enhance.py:848-852); the four
// waves' partials are added in wave order.  stage(c) puts chunk c into Ws and ends with the barrier that makes it
// visible.
template <int NTW, class RS, class Stage>
__device__ __forceinline__ void final_mask(const float* Hs, const float* Ws, float* Lp, const int* valid, RS rs,
                                           float* mask_out, int64_t row0, int64_t rows, int F, int N, int LD,
                                           int tid, int w, int r, int q, Stage&& stage) {
    const int NT = np16(N) >> 4, NC = (F + FC - 1) / FC, rh = N / 2;
    for (int c = 0; c < NC; ++c) {
        stage(c);
        float cl[2], ns[2];
        lambda_partial<NTW, 1>(Hs, Ws, Lp, LD, NT, w, r, q, rh);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int idx = tid + 256 * k;
            const float* p = Lp + (idx >> 5) * LLD + (idx & 31);
            cl[k] = ((p[0] + p[TR * LLD]) + p[2 * TR * LLD]) + p[3 * TR * LLD];
        }
        __syncthreads();
        lambda_partial<NTW, 2>(Hs, Ws, Lp, LD, NT, w, r, q, rh);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int idx = tid + 256 * k, rl = idx >> 5, f = c * FC + (idx & 31);
            const float* p = Lp + rl * LLD + (idx & 31);
            ns[k] = ((p[0] + p[TR * LLD]) + p[2 * TR * LLD]) + p[3 * TR * LLD];
            const int64_t row = row0 + rl;
            if (row < rows && f < F)
                mask_out[row * F + f] = valid[rl] ? cl[k] / (row_scaled(1e-9f, rs, rl) + cl[k] + ns[k]) : 0.f;
        }
        __syncthreads();
    }
}

// A tile without a valid row has nothing to compute: its rows' masks are 0.  True when that was the case.
__device__ __forceinline__ bool all_masked(const int* valid, float* mask_out, int64_t row0, int64_t rows, int F,
                                           int tid) {
    int nvalid = 0;
#pragma unroll
    for (int i = 0; i < TR; ++i) nvalid += valid[i];
    if (nvalid != 0) return false;
    for (int rl = 0; rl < TR; ++rl) {
        const int64_t row = row0 + rl;
        if (row >= rows) break;
        for (int f = tid; f < F; f += 256) mask_out[row * F + f] = 0.f;
    }
    return true;
}

// Launch of a tile kernel instance on `grid` workgroups of 256.  Once per instance and device: the dynamic-LDS
// limit of the widest shape the instance takes (lds_max; a property of the function, not of a launch; a second
// thread that gets here first sets the same value again).
template <auto Kern, class... Args>
hipError_t launch_grid(int device, size_t lds_max, size_t lds, dim3 grid, hipStream_t stream, Args... args) {
    static std::atomic<bool> raised[64];
    if (device < 0 || device >= 64 || !raised[device].load(std::memory_order_acquire)) {
        const hipError_t e = hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds_max);
        if (e != hipSuccess) return e;
        if (device >= 0 && device < 64) raised[device].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(Kern, grid, dim3(256), lds, stream, args...);
    return hipGetLastError();
}

// ... 16 rows per workgroup
template <auto Kern, class... Args>
hipError_t launch(int device, size_t lds_max, size_t lds, int64_t rows, hipStream_t stream, Args... args) {
    return launch_grid<Kern>(device, lds_max, lds, dim3((unsigned)((rows + TR - 1) / TR)), stream, args...);
}

// ---- host side -------------------------------------------------------------------------------------------------

// f(16-column tiles per wave, VEC) as two integral constants: 4 tiles up to N = 256, 8 up to MAX_N
template <class Fn>
auto with_instance(int N, bool vec, Fn&& f) {
    using W4 = std::integral_constant<int, 4>;
    using W8 = std::integral_constant<int, 8>;
    if (np16(N) <= 256) return vec ? f(W4{}, std::true_type{}) : f(W4{}, std::false_type{});
    return vec ? f(W8{}, std::true_type{}) : f(W8{}, std::false_type{});
}
// the dynamic-LDS limit of an instance: the size at the widest N it takes
constexpr int widest_n(int NTW) { return NTW == 4 ? 256 : MAX_N; }

// The argument checks that every forward entry makes, `name` in front of the message; DRNMF_OK or the error's code.
// Three calls and not one: every entry has checks of its own between them (path; n0 and B; v_floor; alignment), and
// which error wins when two apply stays as it was.
inline int32_t check_shape(drnmf_handle_t h, const char* name, int B, int T, int F, int N, int n_iter) {
    if (B <= 0 || T <= 0 || F <= 0 || N <= 0 || n_iter < 0)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: bad shape B=%d T=%d F=%d N=%d iters=%d", name, B, T, F, N, n_iter);
    if (N % 2)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: N = %d must be even (speech and noise halves)", name, N);
    return DRNMF_OK;
}
inline int32_t check_flags(drnmf_handle_t h, const char* name, float sparsity, int has_mask) {
    if (!(sparsity >= 0.f) || (has_mask != 0 && has_mask != 1))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: sparsity must be >= 0, has_mask 0 or 1", name);
    return DRNMF_OK;
}
inline int32_t check_pointers(drnmf_handle_t h, const char* name, std::initializer_list<const void*> required) {
    for (const void* p : required)
        if (!p) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: NULL pointer argument", name);
    return DRNMF_OK;
}

}  // namespace snmf_tile
