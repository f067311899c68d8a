// The sparse-NMF baseline's inference under the Kullback-Leibler cost (cf 'kl', beta == 1; include/drnmf_snmf_kl.h;
// sparse_nmf_gpu.m:201-205, 212-216, 228) on the tile kernel's structure (snmf_mask.hip): one workgroup of four
// waves takes 16 frame rows through all n_iter iterations, H in LDS, the dictionary staged 32 bins at a time
// through a register prefetch, exact-fp32 MFMA.  The phases, the slot map and the LDS layout are snmf_tile.h's.
//
// Against beta == 2 the roles of the two accumulators are swapped:
//     den[n]   = max(sum_f Wn[f][n] + sparsity, flr)      loop invariant and the same for every frame: ONE float per
//                                                         owned column per lane, from a prologue pass that runs
//                                                         `accumulate` on an all-ones operand (the column sums in the
//                                                         kernel's own fmaf order)
//     per chunk c:  Lambda_c = max(H Wc^T, flr)           the four waves' partials added in wave order, as today
//                   num     += (V_c ./ Lambda_c) Wc       the quotient sits in the (q, e) slots Lambda_c had
//     after the last chunk:  H <- H * num / den
// so the numerator is what varies, and it needs the frame's V again in every iteration.
//
// Where V lives: in registers, a chunk at a time.  Lane (r, q) needs exactly the eight values of row r in its
// own slots (bin_base), so it reads them from x itself -- the tile's 16 x F floats stay in L2 -- right after the
// previous chunk's second product, under the next chunk's staging and first product.  Eight
// registers, paid for by the twelve that the one-float-per-column denominator frees; no LDS beyond the Euclidean
// kernel's, so three workgroups of the shipped N = 200 still share a CU.  V = x^power on valid rows and f < F, its
// zeros raised to *v_floor there; everywhere else V = 0 and H = 0, and 0 / flr = 0 rides along without a NaN.
//
// The floor: *v_floor is written in front of the tile kernel, by snmf_kl_floor_init_kernel (the caller's constant)
// or by that and snmf_kl_min_positive_kernel (the reference's rule: the smallest positive V of the call's valid
// rows; +inf = "no positive entry" is read as 0: nothing is raised).
#include "snmf_tile.h"

#include "../../include/drnmf_snmf_kl.h"

namespace {

using namespace snmf_tile;

// The model's 'auto' takes this kernel up to this many rows: the largest measured row count at which it was faster
// than the GEMM path at beta == 1.  Measured (tools/snmf_bench.py --beta 1, MI355X, F = 257, N = 200, 200 iterations,
// this kernel against the GEMM path): 5.08 / 9.35 ms at 32 rows, 5.21 / 10.21 at 4096, 6.90 / 10.42 at 8192, 13.21 /
// 11.09 at 16384, 178.8 / 138.9 at 262144 (DESIGN.md section 6h has the table and the session).  Mirrored by
// _capi.SNMF_KL_AUTO_MAX_ROWS.
constexpr int64_t KL_AUTO_MAX_ROWS = 8192;
constexpr size_t KL_WS_BYTES = 256;           // the floor scalar

// *dst = v: the caller's floor, or +inf in front of the min-positive pass
__global__ void snmf_kl_floor_init_kernel(float* __restrict__ dst, float v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *dst = v;
}

// The reference's floor (sparse_nmf_gpu.m:201-205): the smallest positive V = x^power over the call's valid rows,
// as the bit pattern of a positive float (snmf.hip: min_positive_kernel's atomicMin).  One wave per row, rows
// strided over the grid, one atomic per wave.
__global__ void __launch_bounds__(256)
snmf_kl_min_positive_kernel(const float* __restrict__ x, int64_t rows, int F, float power, float mask_value,
                            int has_mask, unsigned* __restrict__ out_bits) {
    const int l = threadIdx.x & 63;
    const float inf = __int_as_float(0x7f800000);
    float m = inf;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
        const float* src = x + row * F;
        bool any = !has_mask;
        float mr = inf;
        for (int f = l; f < F; f += 64) {
            const float xv = src[f];
            any |= (xv != mask_value);
            const float v = vpow(xv, power);
            if (v > 0.f && v < mr) mr = v;
        }
        if (__any(any)) m = fminf(m, mr);
    }
    for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o, 64));
    if (l == 0 && m < inf) atomicMin(out_bits, __float_as_uint(m));     // positive floats order as their bits
}

// NTW, VEC and the waves per SIMD: as snmf_mask_tile_kernel's.  POW: a spectrogram power other than 1 and 2 -- powf
// sits in the chunk loop then, eight times a chunk, and its temporaries do not fit beside the rest at three waves
// per SIMD (168 VGPRs: 8 bytes of scratch), so those instances are compiled for two.
template <int NTW, bool VEC, bool POW>
__global__ void __launch_bounds__(256, NTW == 4 ? (POW ? 2 : 3) : 1)
snmf_kl_tile_kernel(const float* __restrict__ x, const float* __restrict__ Wn, const float* __restrict__ h_init,
                    const float* __restrict__ v_floor, float* __restrict__ mask_out, int64_t rows, int F, int N,
                    int n_iter, float sparsity, float power, float mask_value, int has_mask) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Np = np16(N), NT = Np >> 4, LD = Np + 8, NC = (F + FC - 1) / FC;
    float* Hs = smem;                         // [TR][LD]   current H (first product's A operand)
    float* Ws = Hs + TR * LD;                 // [FC][LD]   dictionary chunk, zero behind F and N
    float* Lp = Ws + FC * LD;                 // [4][TR][LLD] per-wave partials of Lambda_c
    int* valid = (int*)(Lp + 4 * TR * LLD);   // [TR]
    const int tid = threadIdx.x, l = tid & 63, r = l & 15, q = l >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * TR;
    const float flr = 1e-9f;                  // sparse_nmf_gpu.m:172

    row_validity(x, valid, row0, rows, F, mask_value, has_mask, w, l);
    __syncthreads();
    if (all_masked(valid, mask_out, row0, rows, F, tid)) return;

    float vfl = *v_floor;
    if (!(vfl < __int_as_float(0x7f800000))) vfl = 0.f;          // no positive entry in the call: nothing is raised

    init_h<NTW>(Hs, h_init, valid, N, NT, LD, w, r, q);
    f32x4 num[NTW];
    float den[NTW];
#pragma unroll
    for (int i = 0; i < NTW; ++i) num[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    // this lane's eight values of V in chunk c: row r, slots (q, e) of both k-steps
    const bool rv = valid[r] != 0;            // (a valid row lies inside the call)
    const float* xr = x + (rv ? (row0 + r) * F : 0);
    float vF[2][4];
    auto vload = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int f = c * FC + 16 * s + bin_base(q) + (e & 1) + 4 * (e >> 1);
                float v = xr[f < F ? f : F - 1];                 // (no branch: an invalid row reads x's first)
                if constexpr (POW) v = vpow(v, power);
                else v = power == 2.f ? v * v : v;
                if (v == 0.f) v = vfl;        // sparse_nmf_gpu.m:201-205
                vF[s][e] = (rv && f < F) ? v : 0.f;
            }
    };

    Chunk<NTW, VEC> pf;
    gload(pf, Wn, 0, F, N, w, l);
    // den = max(column sums of Wn + sparsity, flr), once: `accumulate` on an all-ones operand, every row alike
    {
        const float ones[2][4] = {{1.f, 1.f, 1.f, 1.f}, {1.f, 1.f, 1.f, 1.f}};
        for (int c = 0; c < NC; ++c) {
            swrite(pf, Ws, LD, Np, w, l);
            __syncthreads();
            gload(pf, Wn, c + 1 < NC ? c + 1 : 0, F, N, w, l);
            accumulate<NTW>(Ws, LD, NT, w, r, q, ones, num);
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < NTW; ++i) den[i] = fmaxf(num[i][0] + sparsity, flr);
    }
    vload(0);

    for (int it = 0; it < n_iter; ++it) {
#pragma unroll
        for (int i = 0; i < NTW; ++i) num[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < NC; ++c) {
            swrite(pf, Ws, LD, Np, w, l);
            __syncthreads();                  // Ws (and, for c == 0, the new H) visible
            gload(pf, Wn, c + 1 < NC ? c + 1 : 0, F, N, w, l);
            lambda_partial<NTW, 0>(Hs, Ws, Lp, LD, NT, w, r, q, 0);
            __syncthreads();
            float aF[2][4];
            lambda_sum(Lp, r, q, aF);
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int e = 0; e < 4; ++e) aF[s][e] = vF[s][e] / fmaxf(aF[s][e], flr);       // sparse_nmf_gpu.m:213
            accumulate<NTW>(Ws, LD, NT, w, r, q, aF, num);
            vload(c + 1 < NC ? c + 1 : 0);    // the next chunk's V, in flight under that chunk's first product
            __syncthreads();                  // every wave is done with Ws and Lp
        }
        // sparse_nmf_gpu.m:216, on this lane's own elements
        for_own_h<NTW>(NT, w, r, q, [&](int i, int v, int row, int col) {
            float* hp = Hs + row * LD + col;
            *hp = *hp * num[i][v] / den[i];
        });
    }

    final_mask<NTW>(Hs, Ws, Lp, valid, nullptr, mask_out, row0, rows, F, N, LD, tid, w, r, q, [&](int c) {
        swrite(pf, Ws, LD, Np, w, l);
        __syncthreads();
        if (c + 1 < NC) gload(pf, Wn, c + 1, F, N, w, l);
    });
}

}  // namespace

extern "C" int32_t drnmf_snmf_kl_admitted(int32_t F, int32_t N) {
    return (F > 0 && N >= 2 && N <= MAX_N) ? 1 : 0;
}

extern "C" size_t drnmf_snmf_kl_workspace_bytes(void) { return KL_WS_BYTES; }

extern "C" int64_t drnmf_snmf_kl_auto_max_rows(void) { return KL_AUTO_MAX_ROWS; }

extern "C" int32_t drnmf_snmf_kl_forward(drnmf_handle_t h, int32_t B, int32_t T, int32_t F, int32_t N,
                                         int32_t n_iter, float sparsity, float power, float mask_value,
                                         int32_t has_mask, const float* x, const float* Wn, const float* h_init,
                                         float v_floor, float* mask_out, void* workspace, size_t workspace_bytes,
                                         void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (int32_t rc = check_shape(h, "snmf_kl_forward", B, T, F, N, n_iter)) return rc;
    if (int32_t rc = check_flags(h, "snmf_kl_forward", sparsity, has_mask)) return rc;
    if (!(v_floor >= 0.f) || !(v_floor < __builtin_inff()))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "snmf_kl_forward: v_floor = %g must be 0 (the call's smallest positive "
                   "V) or a positive finite constant", (double)v_floor);
    if (int32_t rc = check_pointers(h, "snmf_kl_forward", {x, Wn, h_init, mask_out})) return rc;
    const int64_t rows = (int64_t)B * T;
    if (rows > 0x7fffff00)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "snmf_kl_forward: too many rows (%lld)", (long long)rows);
    if (N > MAX_N)
        DRNMF_FAIL(h, DRNMF_ERR_UNSUPPORTED, "snmf_kl_forward: the kernel takes N <= %d (N = %d)", MAX_N, N);
    if (!workspace || workspace_bytes < KL_WS_BYTES)
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "snmf_kl_forward: workspace %zu < required %zu",
                   workspace ? workspace_bytes : (size_t)0, KL_WS_BYTES);
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "snmf_kl_forward: the handle is bound to no device");
    hipStream_t stream = (hipStream_t)stream_;
    float* vf = (float*)workspace;
    const bool per_call = v_floor == 0.f;
    hipLaunchKernelGGL(snmf_kl_floor_init_kernel, dim3(1), dim3(64), 0, stream, vf,
                       per_call ? __builtin_inff() : v_floor);
    DRNMF_HIP(h, hipGetLastError());
    if (per_call) {
        const int64_t blocks = (rows + 3) / 4;
        hipLaunchKernelGGL(snmf_kl_min_positive_kernel, dim3(blocks > 1024 ? 1024u : (unsigned)blocks), dim3(256), 0,
                           stream, x, rows, F, power, mask_value, has_mask, (unsigned*)vf);
        DRNMF_HIP(h, hipGetLastError());
    }
    const bool vec = N % 4 == 0 && ((uintptr_t)Wn & 15) == 0, pw = power != 1.f && power != 2.f;
    const hipError_t e = with_instance(N, vec, [&](auto ntw, auto v) {
        constexpr int NTW = decltype(ntw)::value;
        constexpr bool VEC = decltype(v)::value;
        auto go = [&](auto pw_) {
            return launch<snmf_kl_tile_kernel<NTW, VEC, decltype(pw_)::value>>(
                h->device, lds_bytes(widest_n(NTW)), lds_bytes(N), rows, stream, x, Wn, h_init, (const float*)vf,
                mask_out, rows, F, N, n_iter, sparsity, power, mask_value, has_mask);
        };
        return pw ? go(std::true_type{}) : go(std::false_type{});      // POW: see the kernel
    });
    DRNMF_HIP(h, e);
    return DRNMF_OK;
}
