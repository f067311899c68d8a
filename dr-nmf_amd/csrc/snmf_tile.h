// The exact-fp32 phases that the sparse-NMF tile kernels share (snmf_mask.hip: snmf_mask_tile_kernel, snmf_f16.hip:
// snmf_f16_tile_kernel): the slot map of the two products, the wave's partial of H Wc^T, acc += A Wc, the
// numerator's chunk, the final-mask loop, the exit of a tile whose rows are all masked, and the launch with its
// dynamic-LDS limit.  What defines the baseline's result is written here once.  A caller may vary: LD (the row
// stride of Hs and Ws), the row scale (rs: nullptr = none, and then no multiply either; else s[rl] multiplies V
// and the mask's epsilon) and how a chunk of the dictionary gets into Ws (a callable).  The per-wave partials in
// Lp are TR * LLD floats apart in both kernels (the fp16 kernel's wider stride is its iterations' own).
// snmf_adapt.hip runs the same phases on a dictionary per batch row.
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
#include <type_traits>

namespace snmf_tile {

constexpr int TR = 16;            // rows per workgroup (one MFMA M-tile)
constexpr int FC = 32;            // bins per staged dictionary chunk
constexpr int LLD = 36;           // row stride of the 16 x 32 partial / V chunk buffers

constexpr int np16(int N) { return (N + 15) & ~15; }

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

}  // namespace snmf_tile
