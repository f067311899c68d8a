// The noise-adaptive sparse-NMF baseline (include/drnmf_snmf_adapt.h): every batch row carries a dictionary of its
// own, W_b [F][N] in the workspace, whose leading n0 atoms stay as they came in and whose other N - n0 follow the
// row's frames (sparse_nmf_gpu.m:210-264 with w_update_ind false on the first n0, beta == 2).  Plain launches on
// the caller's stream, per iteration:
//
//  - snmf_adapt_h_kernel: one workgroup owns 16 frames of one row, with the layout, the stager and the phases of
//    snmf_tile.h.  W_b moves every iteration, so the numerator V W_b is taken again beside the
//    denominator: one pass over W_b's chunks serves both.  H <- H num / max(den + sparsity, flr), stored.
//  - snmf_adapt_stats_kernel: a workgroup owns (a chunk of 32 bins, a block of TB = 64 frames, a row).  Per 16
//    frames it rebuilds Lambda = max(H W_b^T, flr) on chip from the new H (lambda_partial), then contracts V and
//    Lambda with the updated atoms' H over those frames on the matrix pipe:  num [32][Nu] += V^T H_u,
//    den [32][Nu] += Lambda^T H_u.  The block's partials go to P [b][block][2][F][Nu].
//  - snmf_adapt_col_kernel: per row and updated atom, the blocks' partials added in ascending block order, the
//    two column sums, the update, the norm, the guard, the write of W_b's column.
//
// and, after the last iteration, snmf_adapt_final_kernel (final_mask on W_b and H).  No workgroup waits for
// another and nothing is accumulated with atomics.  Exact-fp32 MFMA throughout (the handle's matrix mode does not
// apply).  Order of every sum over frames: a tile is 16 frames and a block 64 frames counted from the row's first
// frame, a masked or padded frame contributes an exact 0, and a block without a valid frame is left out -- so a
// row's bits depend on the row alone.
#include "snmf_tile.h"

#include "../../include/drnmf_snmf_adapt.h"

namespace {

using namespace snmf_tile;

constexpr int TB = 64;            // frames per statistics block (four 16-frame tiles)
constexpr int LS = 48;            // row stride of the stats kernel's V / Lambda tiles: rows 4 s + q, q = 0..3, land
                                  // 16 banks apart for the 16-lane reads of the second product
constexpr float FLR = 1e-9f;      // sparse_nmf_gpu.m:172

// Hs [16][LD] <- H of the frames t0 .. t0 + 15 of the row (Hrow = the row's [T][N]), 0 behind T and N.  Every
// lane loads the elements it owns in the update (row 4 q + v, column 16 t + r).
// (This walk, the H pass's stores and the statistics pass's copy are written out and not through snmf_tile.h's
// for_own_h: with it the iteration measured 0.5 % slower at B = 16)
template <int NTW>
__device__ __forceinline__ void load_h(const float* __restrict__ Hrow, float* Hs, int t0, int T, int N, int LD,
                                       int NT, int w, int r, int q) {
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int t = w + 4 * i, col = 16 * t + r;
        if (t < NT) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int rl = 4 * q + v;
                float hv = 0.f;
                if (col < N && t0 + rl < T) hv = Hrow[(size_t)(t0 + rl) * N + col];
                Hs[rl * LD + col] = hv;
            }
        }
    }
}

// valid [b][t] (keras.layers.Masking's rule), H [b][t][:] = h_init on valid frames and 0 elsewhere, and
// blkany [b][k]: whether block k of the row holds a valid frame.  One workgroup per (block, row).
__global__ void __launch_bounds__(256)
snmf_adapt_prep_kernel(const float* __restrict__ x, const float* __restrict__ h_init, float* __restrict__ H,
                       int* __restrict__ valid, int* __restrict__ blkany, int T, int F, int N, int nblk,
                       float mask_value, int has_mask) {
    __shared__ int cnt[4];
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, k = blockIdx.x, b = blockIdx.y;
    int mine = 0;
    for (int i = w; i < TB; i += 4) {
        const int t = k * TB + i;
        if (t >= T) break;
        const size_t row = (size_t)b * T + t;
        bool any = !has_mask;
        if (has_mask) {
            for (int f = l; f < F; f += 64) any |= (x[row * F + f] != mask_value);
            any = __any(any);
        }
        for (int c = l; c < N; c += 64) H[row * N + c] = any ? h_init[c] : 0.f;
        if (l == 0) valid[row] = any ? 1 : 0;
        mine += any ? 1 : 0;
    }
    if (l == 0) cnt[w] = mine;
    __syncthreads();
    if (threadIdx.x == 0) blkany[(size_t)b * nblk + k] = (cnt[0] + cnt[1] + cnt[2] + cnt[3]) != 0;
}

// every row's dictionary starts as Wn
__global__ void __launch_bounds__(256)
snmf_adapt_bcast_kernel(const float* __restrict__ Wn, float* __restrict__ Wb, int FN) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < FN) Wb[(size_t)blockIdx.y * FN + i] = Wn[i];
}

// Dynamic LDS of the H pass (a V chunk buffer behind Lp) and of the statistics pass (its V and Lambda tiles there)
constexpr size_t h_lds_bytes(int N) { return lds_bytes(N, LLD, TR * LLD + TR); }
constexpr size_t stats_lds_bytes(int N) { return lds_bytes(N, LLD, 2 * TR * LS); }
static_assert(h_lds_bytes(200) == 53056 && stats_lds_bytes(200) == 56832, "as before the sizes were shared");

// One H update of 16 frames of row blockIdx.y against the row's dictionary.  NTW, VEC, the layout and the waves per
// SIMD as in snmf_mask_tile_kernel; Vs is a V chunk buffer of its own because the numerator's chunk and the
// partials of Lambda are alive in the same chunk step.
template <int NTW, bool VEC>
__global__ void __launch_bounds__(256, NTW == 4 ? 3 : 1)
snmf_adapt_h_kernel(const float* __restrict__ x, const float* __restrict__ Wb, float* __restrict__ H,
                    const int* __restrict__ valid_g, int T, int F, int N, float sparsity, float power) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Np = np16(N), NT = Np >> 4, LD = Np + 8, NC = (F + FC - 1) / FC;
    float* Hs = smem;                         // [TR][LD]
    float* Ws = Hs + TR * LD;                 // [FC][LD]
    float* Lp = Ws + FC * LD;                 // [4][TR][LLD]
    float* Vs = Lp + 4 * TR * LLD;            // [TR][LLD]
    int* valid = (int*)(Vs + TR * LLD);       // [TR]
    const int tid = threadIdx.x, l = tid & 63, r = l & 15, q = l >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, t0 = blockIdx.x * TR;
    const int64_t row0 = (int64_t)b * T + t0;
    const float* W = Wb + (size_t)b * F * N;
    float* Hrow = H + (size_t)b * T * N;

    if (tid < TR) valid[tid] = (t0 + tid < T) ? valid_g[row0 + tid] : 0;
    __syncthreads();
    int nvalid = 0;
#pragma unroll
    for (int i = 0; i < TR; ++i) nvalid += valid[i];
    if (nvalid == 0) return;                  // (H is 0 there already)

    Chunk<NTW, VEC> pf;
    gload(pf, W, 0, F, N, w, l);
    load_h<NTW>(Hrow, Hs, t0, T, N, LD, NT, w, r, q);
    f32x4 num[NTW], den[NTW];
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        num[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        den[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int c = 0; c < NC; ++c) {
        swrite(pf, Ws, LD, Np, w, l);
        num_fill(x, Vs, valid, nullptr, row0, F, c, power, tid);
        __syncthreads();                      // Ws, Vs (and, for c == 0, Hs) visible
        gload(pf, W, c + 1 < NC ? c + 1 : 0, F, N, w, l);
        num_accumulate<NTW>(Ws, Vs, LD, NT, w, r, q, num);
        lambda_partial<NTW, 0>(Hs, Ws, Lp, LD, NT, w, r, q, 0);
        __syncthreads();
        float aF[2][4];
        lambda_sum(Lp, r, q, aF);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int e = 0; e < 4; ++e) aF[s][e] = fmaxf(aF[s][e], FLR);
        accumulate<NTW>(Ws, LD, NT, w, r, q, aF, den);
        __syncthreads();                      // every wave is done with Ws, Vs and Lp
    }
#pragma unroll
    for (int i = 0; i < NTW; ++i) {           // sparse_nmf_gpu.m:217-227
        const int t = w + 4 * i, col = 16 * t + r;
        if (t < NT && col < N) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int rl = 4 * q + v;
                if (t0 + rl < T)
                    Hrow[(size_t)(t0 + rl) * N + col] =
                        Hs[rl * LD + col] * num[i][v] / fmaxf(den[i][v] + sparsity, FLR);
            }
        }
    }
}

// This lane's share of the frames t0 .. t0 + 15 of a row for the statistics pass: its elements of H (load_h's
// ownership; 0 behind T and N) and its two elements of the V chunk c (0 on masked frames and behind T and F).
template <int NTW>
__device__ __forceinline__ void fetch_tile(const float* __restrict__ Hrow, const float* __restrict__ xrow,
                                           const int* __restrict__ vrow, float (&hreg)[NTW][4], float (&vreg)[2],
                                           int t0, int c, int T, int F, int N, int NT, float power, int tid, int w,
                                           int r, int q) {
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int t = w + 4 * i, col = 16 * t + r;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int fr = t0 + 4 * q + v;
            hreg[i][v] = (t < NT && col < N && fr < T) ? Hrow[(size_t)fr * N + col] : 0.f;
        }
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int idx = tid + 256 * kk, fr = t0 + (idx >> 5), f = c * FC + (idx & 31);
        vreg[kk] = (fr < T && f < F && vrow[fr]) ? vpow(xrow[(size_t)fr * F + f], power) : 0.f;
    }
}

// The W update's statistics of (bin chunk blockIdx.x, frame block blockIdx.y, row blockIdx.z): the block's share
// of num = V^T H_u and den = Lambda^T H_u, [32 bins][Nu atoms] each.  Wave w owns the 16-atom tiles w, w + 4, ..
// of the updated atoms, both 16-bin halves of the chunk.
template <int NTW, bool VEC>
__global__ void __launch_bounds__(256, NTW == 4 ? 2 : 1)
snmf_adapt_stats_kernel(const float* __restrict__ x, const float* __restrict__ Wb, const float* __restrict__ H,
                        const int* __restrict__ valid_g, const int* __restrict__ blkany, float* __restrict__ P,
                        int T, int F, int N, int n0, int nblk, float power) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Np = np16(N), NT = Np >> 4, LD = Np + 8, Nu = N - n0, NuT = (Nu + 15) >> 4;
    float* Hs = smem;                         // [TR][LD]    H of 16 frames, all atoms
    float* Ws = Hs + TR * LD;                 // [FC][LD]    the chunk's rows of W_b
    float* Lp = Ws + FC * LD;                 // [4][TR][LLD]
    float* As = Lp + 4 * TR * LLD;            // [2][TR][LS] V and Lambda of the 16 frames x 32 bins
    const int tid = threadIdx.x, l = tid & 63, r = l & 15, q = l >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = blockIdx.x, k = blockIdx.y, b = blockIdx.z;
    if (!blkany[(size_t)b * nblk + k]) return;
    const float* W = Wb + (size_t)b * F * N;
    const float* Hrow = H + (size_t)b * T * N;

    {
        Chunk<NTW, VEC> pf;
        gload(pf, W, c, F, N, w, l);
        swrite(pf, Ws, LD, Np, w, l);
    }
    f32x4 an[NTW][2], ad[NTW][2];
#pragma unroll
    for (int i = 0; i < NTW; ++i)
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
            an[i][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
            ad[i][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    // H and V of 16 frames on their way global -> registers -> LDS: the next tile's loads are in flight under this
    // tile's products
    float hreg[NTW][4], vreg[2];
    fetch_tile<NTW>(Hrow, x + (size_t)b * T * F, valid_g + (size_t)b * T, hreg, vreg, k * TB, c, T, F, N, NT, power,
                    tid, w, r, q);
    for (int sub = 0; sub < TB / TR; ++sub) {
        const int t0 = k * TB + sub * TR;
        if (t0 >= T) break;
        __syncthreads();                      // the tile before this one is done with Hs and As
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const int t = w + 4 * i;
            if (t < NT) {
#pragma unroll
                for (int v = 0; v < 4; ++v) Hs[(4 * q + v) * LD + 16 * t + r] = hreg[i][v];
            }
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int idx = tid + 256 * kk;
            As[(idx >> 5) * LS + (idx & 31)] = vreg[kk];
        }
        if (sub + 1 < TB / TR && t0 + TR < T)
            fetch_tile<NTW>(Hrow, x + (size_t)b * T * F, valid_g + (size_t)b * T, hreg, vreg, t0 + TR, c, T, F, N, NT,
                            power, tid, w, r, q);
        __syncthreads();
        lambda_partial<NTW, 0>(Hs, Ws, Lp, LD, NT, w, r, q, 0);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int idx = tid + 256 * kk, rl = idx >> 5, bb = idx & 31;
            const float* p = Lp + rl * LLD + bb;
            As[TR * LS + rl * LS + bb] = fmaxf(((p[0] + p[TR * LLD]) + p[2 * TR * LLD]) + p[3 * TR * LLD], FLR);
        }
        __syncthreads();
        // k-step s holds the frames 4 s + q; a masked frame's H is 0, so its Lambda = flr contributes an exact 0
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int fr = 4 * s + q;
            float av[2], al[2];
#pragma unroll
            for (int jt = 0; jt < 2; ++jt) {
                av[jt] = As[fr * LS + 16 * jt + r];
                al[jt] = As[TR * LS + fr * LS + 16 * jt + r];
            }
#pragma unroll
            for (int i = 0; i < NTW; ++i) {
                const int t = w + 4 * i;
                if (t < NuT) {
                    const int atom = n0 + 16 * t + r;
                    const float hv = atom < N ? Hs[fr * LD + atom] : 0.f;
#pragma unroll
                    for (int jt = 0; jt < 2; ++jt) {
                        an[i][jt] = mfma16(av[jt], hv, an[i][jt]);
                        ad[i][jt] = mfma16(al[jt], hv, ad[i][jt]);
                    }
                }
            }
        }
    }
    float* Pn = P + ((size_t)b * nblk + k) * 2 * F * Nu;
    float* Pd = Pn + (size_t)F * Nu;
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int t = w + 4 * i, atom = 16 * t + r;
        if (t < NuT && atom < Nu) {
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int bin = c * FC + 16 * jt + 4 * q + v;
                    if (bin < F) {
                        Pn[(size_t)bin * Nu + atom] = an[i][jt][v];
                        Pd[(size_t)bin * Nu + atom] = ad[i][jt][v];
                    }
                }
        }
    }
}

constexpr int CL = 64;            // bin lanes of the column pass (16 atoms x 64 lanes = one workgroup of 1024)

// The sum of the bin lanes' values of this thread's atom, in bin-lane order.  Every thread of the workgroup calls it.
__device__ __forceinline__ float col_sum(float* red, float v, int fl, int aj) {
    red[fl * 16 + aj] = v;
    __syncthreads();
    float s = red[aj];
#pragma unroll
    for (int i = 1; i < CL; ++i) s += red[i * 16 + aj];
    return s;
}

// The update of 16 updated atoms of row blockIdx.y (sparse_nmf_gpu.m:232-262).  Thread (fl, aj): atom aj of the
// 16, the bins fl, fl + 64, ..  (64 bin lanes: at B = 1 the pass is a few workgroups whose time is the length of a
// lane's serial walk over its bins and the blocks).  num and den, once summed over the blocks, and then the unnormalised new column,
// wait in block 0's slots of P: every element is read and written by the one thread that owns it.
__global__ void __launch_bounds__(16 * CL)
snmf_adapt_col_kernel(float* __restrict__ Wb, float* __restrict__ P, const int* __restrict__ blkany, int F,
                      int N, int n0, int nblk) {
    __shared__ float red[3][16 * CL];
    const int aj = threadIdx.x & 15, fl = threadIdx.x >> 4, b = blockIdx.y, Nu = N - n0;
    const int j = blockIdx.x * 16 + aj;
    const bool act = j < Nu;
    const int* any = blkany + (size_t)b * nblk;
    int nany = 0;
    for (int k = 0; k < nblk; ++k) nany += any[k];
    if (nany == 0) return;                    // no valid frame: the row's dictionary stays Wn
    float* W = Wb + (size_t)b * F * N + n0 + j;
    float* Pb = P + (size_t)b * nblk * 2 * F * Nu + j;
    const size_t FNu = (size_t)F * Nu;
    float sn = 0.f, sd = 0.f;
    if (act)
        for (int f = fl; f < F; f += CL) {
            float n = 0.f, d = 0.f;
            for (int k = 0; k < nblk; ++k)
                if (any[k]) {
                    n += Pb[(size_t)k * 2 * FNu + (size_t)f * Nu];
                    d += Pb[(size_t)k * 2 * FNu + FNu + (size_t)f * Nu];
                }
            Pb[(size_t)f * Nu] = n;
            Pb[FNu + (size_t)f * Nu] = d;
            const float wv = W[(size_t)f * N];
            sn += n * wv;
            sd += d * wv;
        }
    sn = col_sum(red[0], sn, fl, aj);
    sd = col_sum(red[1], sd, fl, aj);
    float sq = 0.f;
    if (act)
        for (int f = fl; f < F; f += CL) {
            const float n = Pb[(size_t)f * Nu], d = Pb[FNu + (size_t)f * Nu], wv = W[(size_t)f * N];
            const float wnew = wv * (n + sd * wv) / fmaxf(d + sn * wv, FLR);
            Pb[(size_t)f * Nu] = wnew;
            sq += wnew * wnew;
        }
    sq = col_sum(red[2], sq, fl, aj);
    const float nrm = sqrtf(sq);
    // a norm of 0 (a silent row: num and den are 0) or one that is not finite keeps the column as it was
    if (act && nrm > 0.f && nrm <= 3.4028234e38f)
        for (int f = fl; f < F; f += CL) W[(size_t)f * N] = Pb[(size_t)f * Nu] / nrm;
}

// The mask of 16 frames of row blockIdx.y from the row's last dictionary and H
template <int NTW, bool VEC>
__global__ void __launch_bounds__(256, NTW == 4 ? 3 : 1)
snmf_adapt_final_kernel(const float* __restrict__ Wb, const float* __restrict__ H,
                        const int* __restrict__ valid_g, float* __restrict__ mask_out, int T, int F, int N) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Np = np16(N), NT = Np >> 4, LD = Np + 8, NC = (F + FC - 1) / FC;
    float* Hs = smem;
    float* Ws = Hs + TR * LD;
    float* Lp = Ws + FC * LD;
    int* valid = (int*)(Lp + 4 * TR * LLD);
    const int tid = threadIdx.x, l = tid & 63, r = l & 15, q = l >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, t0 = blockIdx.x * TR;
    const int64_t row0 = (int64_t)b * T + t0, rows = (int64_t)b * T + T;
    const float* W = Wb + (size_t)b * F * N;

    if (tid < TR) valid[tid] = (t0 + tid < T) ? valid_g[row0 + tid] : 0;
    __syncthreads();
    if (all_masked(valid, mask_out, row0, rows, F, tid)) return;
    Chunk<NTW, VEC> pf;
    gload(pf, W, 0, F, N, w, l);
    load_h<NTW>(H + (size_t)b * T * N, Hs, t0, T, N, LD, NT, w, r, q);
    final_mask<NTW>(Hs, Ws, Lp, valid, nullptr, mask_out, row0, rows, F, N, LD, tid, w, r, q, [&](int c) {
        swrite(pf, Ws, LD, Np, w, l);
        __syncthreads();
        if (c + 1 < NC) gload(pf, W, c + 1, F, N, w, l);
    });
}

struct AdaptWs {
    size_t off_W, off_H, off_valid, off_any, off_P, total;
    int nblk;
};
AdaptWs adapt_ws(int B, int T, int F, int N, int n0) {
    AdaptWs w;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += round_up_sz(bytes, 256); return at; };
    w.nblk = (T + TB - 1) / TB;
    w.off_W = take((size_t)B * F * N * 4);
    w.off_H = take((size_t)B * T * N * 4);
    w.off_valid = take((size_t)B * T * 4);
    w.off_any = take((size_t)B * w.nblk * 4);
    w.off_P = take((size_t)B * w.nblk * 2 * F * (N - n0) * 4);
    w.total = o;
    return w;
}

struct Call {
    int device;
    hipStream_t stream;
    int B, T, F, N, n0, nblk, n_iter;
    float sparsity, power;
    const float* x;
    float *Wb, *H, *P, *mask_out;
    int *valid, *blkany;
};

template <int NTW, bool VEC>
hipError_t run_iterations(const Call& c) {
    const int wide = widest_n(NTW);
    const dim3 tiles((unsigned)((c.T + TR - 1) / TR), (unsigned)c.B);
    const dim3 sgrid((unsigned)((c.F + FC - 1) / FC), (unsigned)c.nblk, (unsigned)c.B);
    const int Nu = c.N - c.n0;
    hipError_t e;
    for (int it = 0; it < c.n_iter; ++it) {
        e = launch_grid<snmf_adapt_h_kernel<NTW, VEC>>(c.device, h_lds_bytes(wide), h_lds_bytes(c.N), tiles, c.stream,
                                                       c.x, (const float*)c.Wb, c.H, (const int*)c.valid, c.T, c.F,
                                                       c.N, c.sparsity, c.power);
        if (e != hipSuccess) return e;
        if (Nu == 0) continue;
        e = launch_grid<snmf_adapt_stats_kernel<NTW, VEC>>(c.device, stats_lds_bytes(wide), stats_lds_bytes(c.N),
                                                           sgrid, c.stream, c.x, (const float*)c.Wb,
                                                           (const float*)c.H, (const int*)c.valid,
                                                           (const int*)c.blkany, c.P, c.T, c.F, c.N, c.n0, c.nblk,
                                                           c.power);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(snmf_adapt_col_kernel, dim3((unsigned)((Nu + 15) / 16), (unsigned)c.B), dim3(16 * CL), 0,
                           c.stream, c.Wb, c.P, (const int*)c.blkany, c.F, c.N, c.n0, c.nblk);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return launch_grid<snmf_adapt_final_kernel<NTW, VEC>>(c.device, lds_bytes(wide), lds_bytes(c.N), tiles, c.stream,
                                                          (const float*)c.Wb, (const float*)c.H, (const int*)c.valid,
                                                          c.mask_out, c.T, c.F, c.N);
}

bool shape_ok(int B, int T, int F, int N, int n0) {
    return B > 0 && B <= 65535 && T > 0 && F > 0 && N > 0 && N % 2 == 0 && n0 >= 0 && n0 <= N;
}

}  // namespace

extern "C" int32_t drnmf_snmf_adapt_admitted(int32_t F, int32_t N, float beta) {
    return (F > 0 && N >= 2 && N <= MAX_N && beta == 2.f) ? 1 : 0;
}

extern "C" size_t drnmf_snmf_adapt_workspace_bytes(int32_t B, int32_t T, int32_t F, int32_t N, int32_t n0) {
    if (!shape_ok(B, T, F, N, n0) || !drnmf_snmf_adapt_admitted(F, N, 2.f)) return 0;
    return adapt_ws(B, T, F, N, n0).total;
}

extern "C" int32_t drnmf_snmf_adapt_forward(drnmf_handle_t h, int32_t B, int32_t T, int32_t F, int32_t N,
                                            int32_t n0, int32_t n_iter, float sparsity, float power,
                                            float mask_value, int32_t has_mask, const float* x, const float* Wn,
                                            const float* h_init, float* mask_out, float* W_out, float* H_out,
                                            void* workspace, size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (int32_t rc = check_shape(h, "snmf_adapt_forward", B, T, F, N, n_iter)) return rc;
    if (n0 < 0 || n0 > N)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "snmf_adapt_forward: n0 = %d fixed atoms of N = %d", n0, N);
    if (B > 65535) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "snmf_adapt_forward: at most 65535 rows per call (B = %d)", B);
    if (int32_t rc = check_flags(h, "snmf_adapt_forward", sparsity, has_mask)) return rc;
    if (int32_t rc = check_pointers(h, "snmf_adapt_forward", {x, Wn, h_init, mask_out})) return rc;
    if ((int64_t)B * T > 0x7fffff00)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "snmf_adapt_forward: too many frames (%lld)", (long long)B * T);
    if (!drnmf_snmf_adapt_admitted(F, N, 2.f))
        DRNMF_FAIL(h, DRNMF_ERR_UNSUPPORTED, "snmf_adapt_forward: the kernels take 2 <= N <= %d (N = %d)", MAX_N, N);
    const AdaptWs L = adapt_ws(B, T, F, N, n0);
    if (!workspace || workspace_bytes < L.total)
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "snmf_adapt_forward: workspace %zu < required %zu",
                   workspace ? workspace_bytes : (size_t)0, L.total);
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "snmf_adapt_forward: the handle is bound to no device");
    char* ws = (char*)workspace;
    Call c;
    c.device = h->device;
    c.stream = (hipStream_t)stream_;
    c.B = B, c.T = T, c.F = F, c.N = N, c.n0 = n0, c.nblk = L.nblk, c.n_iter = n_iter;
    c.sparsity = sparsity, c.power = power;
    c.x = x;
    c.Wb = (float*)(ws + L.off_W);
    c.H = (float*)(ws + L.off_H);
    c.P = (float*)(ws + L.off_P);
    c.mask_out = mask_out;
    c.valid = (int*)(ws + L.off_valid);
    c.blkany = (int*)(ws + L.off_any);
    hipLaunchKernelGGL(snmf_adapt_prep_kernel, dim3((unsigned)L.nblk, (unsigned)B), dim3(256), 0, c.stream, x, h_init,
                       c.H, c.valid, c.blkany, T, F, N, L.nblk, mask_value, has_mask);
    DRNMF_HIP(h, hipGetLastError());
    hipLaunchKernelGGL(snmf_adapt_bcast_kernel, dim3((unsigned)((F * N + 255) / 256), (unsigned)B), dim3(256), 0,
                       c.stream, Wn, c.Wb, F * N);
    DRNMF_HIP(h, hipGetLastError());
    // (a row's dictionary starts 16-byte aligned when N % 4 == 0)
    const hipError_t e = with_instance(N, N % 4 == 0, [&](auto ntw, auto v) {
        return run_iterations<decltype(ntw)::value, decltype(v)::value>(c);
    });
    DRNMF_HIP(h, e);
    if (W_out)
        DRNMF_HIP(h, hipMemcpyAsync(W_out, c.Wb, (size_t)B * F * N * 4, hipMemcpyDeviceToDevice, c.stream));
    if (H_out)
        DRNMF_HIP(h, hipMemcpyAsync(H_out, c.H, (size_t)B * T * N * 4, hipMemcpyDeviceToDevice, c.stream));
    return DRNMF_OK;
}
