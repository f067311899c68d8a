// The sparse-NMF baseline's inference as one call (include/drnmf_snmf.h; enhance.py:838-852): padded sequences
// x [B][T][F] in, the ratio mask out.  Two paths:
//
//  - the tile kernel (snmf_mask_tile_kernel, beta == 2, N <= 512).  MU inference has no recurrence and no
//    coupling between frames, so one workgroup takes 16 consecutive frame rows through ALL n_iter iterations:
//    the loop-invariant numerator V Wn and the denominator live in registers, H in LDS (the operand of the
//    first product), the dictionary streams from L2 through LDS 32 bins at a time, and Lambda = max(H Wn^T, flr)
//    exists only as that 16 x 32 chunk.  One launch instead of 3 n_iter, nothing but x and the mask in HBM.
//  - the GEMM path: a pack kernel, drnmf_mu_forward's launches as they are (snmf.hip), a kernel that zeroes the
//    masked rows.
//
// Tile kernel, per chunk c of FC = 32 bins (Wc = Wn[32 c .. 32 c + 31][:], staged once, serves both products):
//     Lambda_c = max(H Wc^T, flr)     16 x 32, contraction over the atoms: split over the four waves by
//                                     16-atom blocks, the four partials added in wave order
//     den     += Lambda_c Wc          16 x N, contraction over the chunk's bins: every wave owns the 16-column
//                                     tiles w, w + 4, ... of den, num and H
// and after the last chunk H <- H * num / max(den + sparsity, flr).  Exact-fp32 MFMA (v_mfma_f32_16x16x4_f32: an
// fmaf chain in k order), so a row's result depends on nothing but that row, Wn and h_init: bit for bit the same
// wherever the row sits and whatever its neighbours hold.
//
// LDS: Hs [16][LD], Ws [32][LD], LD = Np + 8 (Np = N rounded up to 16).  snmf_tile.h holds the phases this kernel
// shares with its siblings (snmf_kl.hip, snmf_adapt.hip, snmf_f16.hip), the slot order of the second product and
// why these strides are free of bank conflicts.
#include "snmf_tile.h"

#include "../../include/drnmf_snmf.h"

namespace {

using namespace snmf_tile;

// path = 0 takes the tile kernel up to this many rows: the largest measured row count at which it was the faster
// path.  Measured (tools/snmf_bench.py, MI355X, F = 257, N = 200, 200 iterations, tile against GEMM path): 3.9 / 8.8
// ms at 32 rows, 3.9 / 9.4 at 4096, 5.3 / 9.6 at 8192, 10.35 / 10.18 at 16384, 141.4 / 132.9 at 262144 (DESIGN.md
// section 6h has the table).  Mirrored by _capi.SNMF_TILE_AUTO_MAX_ROWS.
constexpr int64_t TILE_AUTO_MAX_ROWS = 8192;

// NTW: 16-column tiles of H / num / den per wave (4: N <= 256, 8: N <= 512).  VEC: N % 4 == 0 and Wn 16-byte
// aligned -- the dictionary is staged with 16-byte loads.  Waves per SIMD: three workgroups of the shipped N = 200
// share a CU's LDS (51 KB each); the wide form (one workgroup's LDS at N = 512 is 109 KB) takes the registers it
// needs.
template <int NTW, bool VEC>
__global__ void __launch_bounds__(256, NTW == 4 ? 3 : 1)
snmf_mask_tile_kernel(const float* __restrict__ x, const float* __restrict__ Wn,
                      const float* __restrict__ h_init, float* __restrict__ mask_out, int64_t rows, int F,
                      int N, int n_iter, float sparsity, float power, float mask_value, int has_mask) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Np = np16(N), NT = Np >> 4, LD = Np + 8, NC = (F + FC - 1) / FC;
    float* Hs = smem;                         // [TR][LD]   current H (first product's A operand)
    float* Ws = Hs + TR * LD;                 // [FC][LD]   dictionary chunk, zero behind F and N
    float* Lp = Ws + FC * LD;                 // [4][TR][LLD] per-wave partials of Lambda_c; slot 0 also the V chunk
    int* valid = (int*)(Lp + 4 * TR * LLD);   // [TR]
    const int tid = threadIdx.x, l = tid & 63, r = l & 15, q = l >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * TR;
    const float flr = 1e-9f;                  // sparse_nmf_gpu.m:172

    row_validity(x, valid, row0, rows, F, mask_value, has_mask, w, l);
    __syncthreads();
    if (all_masked(valid, mask_out, row0, rows, F, tid)) return;

    // H = h_init on valid rows and the accumulators' zeros in one loop, the Lambda sum and the update below written
    // out: init_h, lambda_sum and for_own_h (snmf_tile.h) say the same, and this kernel measured 0.3 to 0.8 % slower
    // at two workgroups per CU with them
    f32x4 num[NTW], den[NTW];
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int t = w + 4 * i, col = 16 * t + r;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int rl = 4 * q + v;
            float hv = 0.f;
            if (t < NT && col < N && valid[rl]) hv = h_init[col];
            num[i][v] = 0.f;
            den[i][v] = 0.f;
            if (t < NT) Hs[rl * LD + col] = hv;
        }
    }

    Chunk<NTW, VEC> pf;
    gload(pf, Wn, 0, F, N, w, l);
    // num = V Wn, once: V = x^power on valid rows, 0 elsewhere
    for (int c = 0; c < NC; ++c) {
        swrite(pf, Ws, LD, Np, w, l);
        num_fill(x, Lp, valid, nullptr, row0, F, c, power, tid);
        __syncthreads();
        gload(pf, Wn, c + 1 < NC ? c + 1 : 0, F, N, w, l);
        num_accumulate<NTW>(Ws, Lp, LD, NT, w, r, q, num);
        __syncthreads();
    }

    for (int it = 0; it < n_iter; ++it) {
#pragma unroll
        for (int i = 0; i < NTW; ++i) den[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < NC; ++c) {
            swrite(pf, Ws, LD, Np, w, l);
            __syncthreads();                  // Ws (and, for c == 0, the new H) visible
            gload(pf, Wn, c + 1 < NC ? c + 1 : 0, F, N, w, l);
            lambda_partial<NTW, 0>(Hs, Ws, Lp, LD, NT, w, r, q, 0);
            __syncthreads();
            float aF[2][4];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const float* p = Lp + r * LLD + 16 * s + bin_base(q) + 4 * hh;
                    f32x2 sum = *(const f32x2*)p;                 // the four waves' partials, in wave order
                    sum += *(const f32x2*)(p + TR * LLD);
                    sum += *(const f32x2*)(p + 2 * TR * LLD);
                    sum += *(const f32x2*)(p + 3 * TR * LLD);
                    aF[s][2 * hh] = fmaxf(sum[0], flr);
                    aF[s][2 * hh + 1] = fmaxf(sum[1], flr);
                }
            accumulate<NTW>(Ws, LD, NT, w, r, q, aF, den);
            __syncthreads();                  // every wave is done with Ws and Lp
        }
#pragma unroll
        for (int i = 0; i < NTW; ++i) {       // sparse_nmf_gpu.m:217-227
            const int t = w + 4 * i;
            if (t < NT) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    float* hp = Hs + (4 * q + v) * LD + 16 * t + r;      // (this lane's own elements)
                    *hp = *hp * num[i][v] / fmaxf(den[i][v] + sparsity, flr);
                }
            }
        }
    }

    final_mask<NTW>(Hs, Ws, Lp, valid, nullptr, mask_out, row0, rows, F, N, LD, tid, w, r, q, [&](int c) {
        swrite(pf, Ws, LD, Np, w, l);
        __syncthreads();
        if (c + 1 < NC) gload(pf, Wn, c + 1, F, N, w, l);
    });
}

// GEMM path, in front of drnmf_mu_forward: V = x^power (masked rows 0), H = h_init in every valid row, the
// validity flags.  One wave per row.
__global__ void __launch_bounds__(256)
snmf_mask_pack_kernel(const float* __restrict__ x, const float* __restrict__ h_init, float* __restrict__ V,
                      float* __restrict__ H, unsigned char* __restrict__ valid, int64_t rows, int F, int N,
                      float power, float mask_value, int has_mask) {
    const int l = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* src = x + row * F;
    bool any = !has_mask;
    if (has_mask) {
        for (int f = l; f < F; f += 64) any |= (src[f] != mask_value);
        any = __any(any);
    }
    for (int f = l; f < F; f += 64) {
        const float xv = src[f];
        V[row * F + f] = any ? vpow(xv, power) : 0.f;
    }
    for (int c = l; c < N; c += 64) H[row * N + c] = any ? h_init[c] : 0.f;
    if (l == 0) valid[row] = any ? 1 : 0;
}

// ... and behind it: the mask of a masked row is 0
__global__ void __launch_bounds__(256)
snmf_mask_zero_kernel(float* __restrict__ mask_out, const unsigned char* __restrict__ valid, int64_t rows,
                      int F) {
    const int l = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows || valid[row]) return;
    for (int f = l; f < F; f += 64) mask_out[row * F + f] = 0.f;
}

struct MaskWs {
    size_t off_V, off_H, off_W2, off_valid, off_mu, mu_bytes, total;
};
MaskWs mask_ws(int64_t rows, int F, int N) {
    MaskWs w;
    size_t o = 0;
    auto take = [&](size_t b) { size_t at = o; o += round_up_sz(b, 256); return at; };
    w.off_V = take((size_t)rows * F * 4);
    w.off_H = take((size_t)rows * N * 4);
    w.off_W2 = take((size_t)F * N * 4);       // drnmf_mu_forward's normalised copy (of the normalised Wn)
    w.off_valid = take((size_t)rows);
    w.mu_bytes = drnmf_mu_workspace_bytes(rows, F, N);
    w.off_mu = take(w.mu_bytes);
    w.total = o;
    return w;
}

}  // namespace

extern "C" int32_t drnmf_snmf_mask_admitted(int32_t F, int32_t N, float beta) {
    return (F > 0 && N >= 2 && N <= MAX_N && beta == 2.f) ? 1 : 0;
}

extern "C" size_t drnmf_snmf_mask_workspace_bytes(int32_t B, int32_t T, int32_t F, int32_t N) {
    if (B <= 0 || T <= 0 || F <= 0 || N <= 0 || N % 2) return 0;
    return mask_ws((int64_t)B * T, F, N).total;
}

extern "C" int32_t drnmf_snmf_mask_forward(drnmf_handle_t h, int32_t B, int32_t T, int32_t F, int32_t N,
                                           int32_t n_iter, float beta, float sparsity, float power,
                                           float mask_value, int32_t has_mask, const float* x, const float* Wn,
                                           const float* h_init, float* mask_out, int32_t path, void* workspace,
                                           size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (int32_t rc = check_shape(h, "snmf_mask_forward", B, T, F, N, n_iter)) return rc;
    if (path < DRNMF_SNMF_PATH_AUTO || path > DRNMF_SNMF_PATH_TILE)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "snmf_mask_forward: unknown path %d", path);
    if (int32_t rc = check_flags(h, "snmf_mask_forward", sparsity, has_mask)) return rc;
    if (int32_t rc = check_pointers(h, "snmf_mask_forward", {x, Wn, h_init, mask_out})) return rc;
    const int64_t rows = (int64_t)B * T;
    if (rows > 0x7fffff00)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "snmf_mask_forward: too many rows (%lld)", (long long)rows);
    const bool admitted = drnmf_snmf_mask_admitted(F, N, beta) != 0;
    if (path == DRNMF_SNMF_PATH_TILE && !admitted)
        DRNMF_FAIL(h, DRNMF_ERR_UNSUPPORTED, "snmf_mask_forward: the tile kernel takes beta == 2 and N <= %d "
                   "(beta = %g, N = %d)", MAX_N, (double)beta, N);
    hipStream_t stream = (hipStream_t)stream_;
    const bool gemm = !(path == DRNMF_SNMF_PATH_TILE ||
                        (path == DRNMF_SNMF_PATH_AUTO && admitted && rows <= TILE_AUTO_MAX_ROWS));
    const MaskWs L = mask_ws(rows, F, N);
    if (gemm && (!workspace || workspace_bytes < L.total))
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "snmf_mask_forward: workspace %zu < required %zu",
                   workspace ? workspace_bytes : (size_t)0, L.total);
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "snmf_mask_forward: the handle is bound to no device");
    if (!gemm) {
        const bool vec = N % 4 == 0 && ((uintptr_t)Wn & 15) == 0;
        const hipError_t e = with_instance(N, vec, [&](auto ntw, auto v) {
            constexpr int NTW = decltype(ntw)::value;
            return launch<snmf_mask_tile_kernel<NTW, decltype(v)::value>>(
                h->device, lds_bytes(widest_n(NTW)), lds_bytes(N), rows, stream, x, Wn, h_init, mask_out, rows, F, N,
                n_iter, sparsity, power, mask_value, has_mask);
        });
        DRNMF_HIP(h, e);
        return DRNMF_OK;
    }
    char* ws = (char*)workspace;
    float* V = (float*)(ws + L.off_V);
    float* H = (float*)(ws + L.off_H);
    float* W2 = (float*)(ws + L.off_W2);
    unsigned char* valid = (unsigned char*)(ws + L.off_valid);
    const dim3 rgrid((unsigned)((rows + 3) / 4));
    hipLaunchKernelGGL(snmf_mask_pack_kernel, rgrid, dim3(256), 0, stream, x, h_init, V, H, valid, rows, F, N,
                       power, mask_value, has_mask);
    DRNMF_HIP(h, hipGetLastError());
    // (Wn's columns have unit norm already: the normalisation in front of the loop rescales by 1 up to rounding)
    const int32_t rc = drnmf_mu_forward(h, rows, F, N, n_iter, beta, sparsity, V, Wn, W2, H, mask_out,
                                        ws + L.off_mu, L.mu_bytes, stream_);
    if (rc != DRNMF_OK) return rc;
    if (has_mask) {
        hipLaunchKernelGGL(snmf_mask_zero_kernel, rgrid, dim3(256), 0, stream, mask_out, valid, rows, F);
        DRNMF_HIP(h, hipGetLastError());
    }
    return DRNMF_OK;
}
