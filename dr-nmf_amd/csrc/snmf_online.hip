// The online noise-adaptive sparse-NMF baseline (include/drnmf_snmf_online.h): every batch row is a stream with a
// dictionary of its own, which moves once per block of L valid frames from the sufficient statistics A = sum H^T H_u
// and Bm = sum V^T H_u of the blocks so far.  The host does not know the rows' counts, so a call of T frames runs a
// number of steps fixed by T and L, S = (T + 2 L - 2) / L (a row that starts in the last slot of a block touches that
// many blocks); step s of a row is the s-th block the call touches, and a row with nothing to do in a step leaves
// early.  Plain launches on the caller's stream:
//
//  per call   snmf_online_valid_kernel   validity of every frame; masked frames' mask and H_out are 0
//             snmf_online_scan_kernel    per row: the positions of its valid frames in order, their number, the phase
//                                        count % L the call starts at; count += number
//  per step   snmf_online_gather_kernel  the row's frames of the step's block into the state's block buffer V [L][F],
//                                        slot = (valid frame's index) % L, and the slots' to-do flags
//             snmf_online_h_kernel       16 slots per workgroup through all n_iter iterations on the row's dictionary:
//                                        the fixed tile kernel's loop on the phases of snmf_tile.h; H into the block
//                                        buffer H [L][N], the masks into a staging block
//             snmf_online_scatter_kernel masks and H of the to-do slots to their frames of mask_out / H_out
//    for the rows whose block is now full (N > n0):
//             snmf_online_stats_kernel   [H | V]^T H_u over the L slots on the matrix pipe, in slot order;
//                                        A <- forget A + .., Bm <- forget Bm + ..
//             w_iter times  snmf_online_col_kernel     den = W A on chip, the batch mode's column update and guard;
//                                                      the new columns go to a buffer beside the dictionary
//                           snmf_online_commit_kernel  .. and from there into the dictionary: every workgroup of the
//                                                      column pass has read the previous iteration's W by then
//
// No workgroup waits for another, nothing is accumulated with atomics, every element of the state has one writer per
// launch.  Exact-fp32 MFMA (the handle's matrix mode does not apply).  A slot's H and mask depend on that frame, the
// row's dictionary and h_init alone (snmf_mask.hip), a slot is computed in the one call that brings its frame, and the
// statistics add the L slots in slot order: a row's bits do not depend on how its frames were cut into calls, on B,
// on T or on the rows beside it.
#include "snmf_tile.h"

#include "../../include/drnmf_snmf_online.h"

namespace {

using namespace snmf_tile;

constexpr int LS = 48;            // row stride of the statistics kernel's left-operand tile (snmf_adapt.hip's LS)
constexpr float FLR = 1e-9f;      // sparse_nmf_gpu.m:172
constexpr int CL = 64;            // bin lanes of the column pass (16 atoms x 64 lanes = one workgroup of 1024)
constexpr int MIN_BLOCK = 16, MAX_BLOCK = 256;

// Does step s of this call complete the row's block?  (ph: the phase the call starts at, n: the call's valid frames)
__device__ __forceinline__ bool block_full(const int* __restrict__ ph, const int* __restrict__ nn, int b, int s,
                                           int L) {
    return ph[b] + nn[b] >= (s + 1) * L;
}

// valid [b][t] (keras.layers.Masking's rule); a masked frame's mask and H_out are 0.  One wave per frame.
__global__ void __launch_bounds__(256)
snmf_online_valid_kernel(const float* __restrict__ x, int* __restrict__ valid, float* __restrict__ mask_out,
                         float* __restrict__ H_out, int T, int F, int N, float mask_value, int has_mask) {
    const int l = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (t >= T) return;
    const size_t row = (size_t)b * T + t;
    bool any = !has_mask;
    if (has_mask) {
        for (int f = l; f < F; f += 64) any |= (x[row * F + f] != mask_value);
        any = __any(any);
    }
    if (l == 0) valid[row] = any ? 1 : 0;
    if (any) return;
    for (int f = l; f < F; f += 64) mask_out[row * F + f] = 0.f;
    if (H_out)
        for (int c = l; c < N; c += 64) H_out[row * N + c] = 0.f;
}

// Row blockIdx.x: pos [b][p] = the frame of its p-th valid frame of the call, nn [b] their number, ph [b] the phase
// the call starts at; the row's count moves on.  Thread i owns the frames i per .. i per + per - 1.
__global__ void __launch_bounds__(256)
snmf_online_scan_kernel(const int* __restrict__ valid, int* __restrict__ pos, int* __restrict__ ph,
                        int* __restrict__ nn, long long* __restrict__ count, int T, int L) {
    __shared__ int part[256];
    const int tid = threadIdx.x, b = blockIdx.x, per = (T + 255) / 256;
    const int t0 = min(T, tid * per), t1 = min(T, t0 + per);
    const int* v = valid + (size_t)b * T;
    int c = 0;
    for (int t = t0; t < t1; ++t) c += v[t];
    part[tid] = c;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) {
            const int m = part[i];
            part[i] = run;
            run += m;
        }
        nn[b] = run;
        ph[b] = (int)(count[b] % L);
        count[b] += run;
    }
    __syncthreads();
    int p = part[tid];
    for (int t = t0; t < t1; ++t)
        if (v[t]) pos[(size_t)b * T + p++] = t;
}

// Slot blockIdx.x of row blockIdx.y in step s: the call's valid frame p = s L + slot - phase, if the call has it, goes
// into the block buffer; todo = its frame + 1, else 0.
__global__ void __launch_bounds__(64)
snmf_online_gather_kernel(const float* __restrict__ x, const int* __restrict__ pos, const int* __restrict__ ph,
                          const int* __restrict__ nn, int* __restrict__ todo, float* __restrict__ Vblk, int s,
                          int T, int F, int L) {
    const int j = blockIdx.x, b = blockIdx.y, p = s * L + j - ph[b];
    const bool mine = p >= 0 && p < nn[b];
    const int t = mine ? pos[(size_t)b * T + p] : -1;
    if (threadIdx.x == 0) todo[(size_t)b * L + j] = t + 1;
    if (!mine) return;
    const float* src = x + ((size_t)b * T + t) * F;
    float* dst = Vblk + ((size_t)b * L + j) * F;
    for (int f = threadIdx.x; f < F; f += 64) dst[f] = src[f];
}

// All n_iter iterations and the mask of 16 slots of row blockIdx.y on the row's dictionary: snmf_mask_tile_kernel's
// loop with the block buffer as x, the to-do flags as validity and a stager that reads W_b.  NTW and VEC as there.
// Two waves per SIMD, not its three: the grid is L / 16 workgroups per row, far fewer than the CUs can hold, and with
// the block buffer's pointers beside the loop's registers the third costs scratch.  A slot that is not to do (empty,
// or done by an earlier call) is a masked row: nothing of it is written.
template <int NTW, bool VEC>
__global__ void __launch_bounds__(256, NTW == 4 ? 2 : 1)
snmf_online_h_kernel(const float* __restrict__ Vblk, const float* __restrict__ Wb, const float* __restrict__ h_init,
                     const int* __restrict__ todo, float* __restrict__ Hblk, float* __restrict__ Mst, int L, int F,
                     int N, int n_iter, float sparsity, float power) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Np = np16(N), NT = Np >> 4, LD = Np + 8, NC = (F + FC - 1) / FC;
    float* Hs = smem;                         // [TR][LD]
    float* Ws = Hs + TR * LD;                 // [FC][LD]
    float* Lp = Ws + FC * LD;                 // [4][TR][LLD]
    int* valid = (int*)(Lp + 4 * TR * LLD);   // [TR]
    const int tid = threadIdx.x, l = tid & 63, r = l & 15, q = l >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    const int64_t row0 = (int64_t)b * L + blockIdx.x * TR, rows = (int64_t)b * L + L;
    const float* W = Wb + (size_t)b * F * N;

    if (tid < TR) valid[tid] = todo[row0 + tid] != 0;      // (L is a multiple of 16: every slot of the tile exists)
    __syncthreads();
    int nvalid = 0;
#pragma unroll
    for (int i = 0; i < TR; ++i) nvalid += valid[i];
    if (nvalid == 0) return;

    init_h<NTW>(Hs, h_init, valid, N, NT, LD, w, r, q);
    f32x4 num[NTW], den[NTW];
#pragma unroll
    for (int i = 0; i < NTW; ++i) num[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    Chunk<NTW, VEC> pf;
    gload(pf, W, 0, F, N, w, l);
    for (int c = 0; c < NC; ++c) {            // num = V W_b, once
        swrite(pf, Ws, LD, Np, w, l);
        num_fill(Vblk, Lp, valid, nullptr, row0, F, c, power, tid);
        __syncthreads();
        gload(pf, W, c + 1 < NC ? c + 1 : 0, F, N, w, l);
        num_accumulate<NTW>(Ws, Lp, LD, NT, w, r, q, num);
        __syncthreads();
    }
    for (int it = 0; it < n_iter; ++it) {
#pragma unroll
        for (int i = 0; i < NTW; ++i) den[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < NC; ++c) {
            swrite(pf, Ws, LD, Np, w, l);
            __syncthreads();                  // Ws (and, for c == 0, the new H) visible
            gload(pf, W, c + 1 < NC ? c + 1 : 0, F, N, w, l);
            lambda_partial<NTW, 0>(Hs, Ws, Lp, LD, NT, w, r, q, 0);
            __syncthreads();
            float aF[2][4];
            lambda_sum(Lp, r, q, aF);
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int e = 0; e < 4; ++e) aF[s][e] = fmaxf(aF[s][e], FLR);
            accumulate<NTW>(Ws, LD, NT, w, r, q, aF, den);
            __syncthreads();                  // every wave is done with Ws and Lp
        }
        for_own_h<NTW>(NT, w, r, q, [&](int i, int v, int row, int col) {     // sparse_nmf_gpu.m:217-227
            float* hp = Hs + row * LD + col;
            *hp = *hp * num[i][v] / fmaxf(den[i][v] + sparsity, FLR);
        });
    }
    for_own_h<NTW>(NT, w, r, q, [&](int, int, int row, int col) {
        if (col < N && valid[row]) Hblk[(row0 + row) * N + col] = Hs[row * LD + col];
    });
    final_mask<NTW>(Hs, Ws, Lp, valid, nullptr, Mst, row0, rows, F, N, LD, tid, w, r, q, [&](int c) {
        swrite(pf, Ws, LD, Np, w, l);
        __syncthreads();
        if (c + 1 < NC) gload(pf, W, c + 1, F, N, w, l);
    });
}

// Slot blockIdx.x of row blockIdx.y: a to-do slot's mask and H go to its frame
__global__ void __launch_bounds__(64)
snmf_online_scatter_kernel(const int* __restrict__ todo, const float* __restrict__ Mst,
                           const float* __restrict__ Hblk, float* __restrict__ mask_out, float* __restrict__ H_out,
                           int T, int F, int N, int L) {
    const size_t slot = (size_t)blockIdx.y * L + blockIdx.x;
    const int t1 = todo[slot];
    if (t1 == 0) return;
    const size_t row = (size_t)blockIdx.y * T + (t1 - 1);
    for (int f = threadIdx.x; f < F; f += 64) mask_out[row * F + f] = Mst[slot * F + f];
    if (H_out)
        for (int c = threadIdx.x; c < N; c += 64) H_out[row * N + c] = Hblk[slot * N + c];
}

// The statistics of a row whose block step s completes: 32 rows of [H | V]^T H_u, [32][Nu], summed over the L slots
// in slot order, then A / Bm <- forget A / Bm + that.  blockIdx.x: the cA chunks of A's N rows, then the chunks of
// Bm's F rows; blockIdx.y: the row.  Wave w owns the 16-atom tiles w, w + 4, .. of the updated atoms, both 16-row
// halves of the chunk (snmf_adapt_stats_kernel's second product and slot map: k-step s4 holds the slots 4 s4 + q).
template <int NTW>
__global__ void __launch_bounds__(256, NTW == 4 ? 2 : 1)
snmf_online_stats_kernel(const float* __restrict__ Vblk, const float* __restrict__ Hblk, float* __restrict__ A,
                         float* __restrict__ Bm, const int* __restrict__ ph, const int* __restrict__ nn, int s, int L,
                         int F, int N, int n0, float forget, float power) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Np = np16(N), LD = Np + 8, Nu = N - n0, NuT = (Nu + 15) >> 4, cA = (N + FC - 1) / FC;
    float* Hs = smem;                         // [TR][LD]  H of 16 slots, all atoms
    float* As = Hs + TR * LD;                 // [TR][LS]  the chunk's 32 rows of [H | V] at those slots
    const int tid = threadIdx.x, l = tid & 63, r = l & 15, q = l >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    if (!block_full(ph, nn, b, s, L)) return;
    const bool isA = (int)blockIdx.x < cA;
    const int base = FC * (isA ? (int)blockIdx.x : (int)blockIdx.x - cA), lim = isA ? N : F;
    const float* Hrow = Hblk + (size_t)b * L * N;
    const float* Vrow = Vblk + (size_t)b * L * F;

    f32x4 acc[NTW][2];
#pragma unroll
    for (int i = 0; i < NTW; ++i)
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) acc[i][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int sub = 0; sub < L / TR; ++sub) {
        const int s0 = sub * TR;
        __syncthreads();                      // the tile before this one is done with Hs and As
        for (int rl = 0; rl < TR; ++rl)
            for (int col = tid; col < Np; col += 256)
                Hs[rl * LD + col] = col < N ? Hrow[(size_t)(s0 + rl) * N + col] : 0.f;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int idx = tid + 256 * kk, rl = idx >> 5, g = base + (idx & 31);
            float v = 0.f;
            if (g < lim) v = isA ? Hrow[(size_t)(s0 + rl) * N + g] : vpow(Vrow[(size_t)(s0 + rl) * F + g], power);
            As[rl * LS + (idx & 31)] = v;
        }
        __syncthreads();
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int fr = 4 * s4 + q;
            float av[2];
#pragma unroll
            for (int jt = 0; jt < 2; ++jt) av[jt] = As[fr * LS + 16 * jt + r];
#pragma unroll
            for (int i = 0; i < NTW; ++i) {
                const int t = w + 4 * i;
                if (t < NuT) {
                    const int atom = n0 + 16 * t + r;
                    const float hv = atom < N ? Hs[fr * LD + atom] : 0.f;
#pragma unroll
                    for (int jt = 0; jt < 2; ++jt) acc[i][jt] = mfma16(av[jt], hv, acc[i][jt]);
                }
            }
        }
    }
    float* dst = isA ? A + (size_t)b * N * Nu : Bm + (size_t)b * F * Nu;
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int t = w + 4 * i, atom = 16 * t + r;
        if (t < NuT && atom < Nu) {
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int g = base + 16 * jt + 4 * q + v;
                    if (g < lim) {
                        float* p = dst + (size_t)g * Nu + atom;
                        *p = forget * *p + acc[i][jt][v];
                    }
                }
        }
    }
}

// The sum of the bin lanes' values of this thread's atom, in bin-lane order.  Every thread of the workgroup calls it.
__device__ __forceinline__ float col_sum(float* red, float v, int fl, int aj) {
    red[fl * 16 + aj] = v;
    __syncthreads();
    float s = red[aj];
#pragma unroll
    for (int i = 1; i < CL; ++i) s += red[i * 16 + aj];
    return s;
}

// One update of 16 updated atoms of row blockIdx.y from the statistics (snmf_adapt_col_kernel with num = Bm and
// den = W A, the contraction over the atoms in atom order with A's 16 columns in LDS).  Thread (fl, aj): atom aj of
// the 16, the bins fl, fl + 64, ..  It reads the dictionary and writes the new columns -- the old one where the
// guard holds it back -- to Wt [b][F][Nu]; den waits in D [b][F][Nu], the unnormalised column in Wt, every element
// with the one thread that owns it.
__global__ void __launch_bounds__(16 * CL)
snmf_online_col_kernel(const float* __restrict__ Wb, const float* __restrict__ A, const float* __restrict__ Bm,
                       float* __restrict__ Wt, float* __restrict__ D, const int* __restrict__ ph,
                       const int* __restrict__ nn, int s, int L, int F, int N, int n0) {
    __shared__ float red[3][16 * CL];
    extern __shared__ __attribute__((aligned(16))) float Ac[];         // [N][16]
    const int aj = threadIdx.x & 15, fl = threadIdx.x >> 4, b = blockIdx.y, Nu = N - n0;
    if (!block_full(ph, nn, b, s, L)) return;
    const int j = blockIdx.x * 16 + aj;
    const bool act = j < Nu;
    const float* Ab = A + (size_t)b * N * Nu;
    for (int idx = threadIdx.x; idx < N * 16; idx += 16 * CL) {
        const int jj = blockIdx.x * 16 + (idx & 15);
        Ac[idx] = jj < Nu ? Ab[(size_t)(idx >> 4) * Nu + jj] : 0.f;
    }
    __syncthreads();
    const float* W = Wb + (size_t)b * F * N;
    const float* num = Bm + (size_t)b * F * Nu + j;
    float* den = D + (size_t)b * F * Nu + j;
    float* out = Wt + (size_t)b * F * Nu + j;
    float sn = 0.f, sd = 0.f;
    if (act)
        for (int f = fl; f < F; f += CL) {
            const float* wr = W + (size_t)f * N;
            float d = 0.f;
            for (int k = 0; k < N; ++k) d = fmaf(wr[k], Ac[k * 16 + aj], d);
            den[(size_t)f * Nu] = d;
            const float wv = wr[n0 + j];
            sn += num[(size_t)f * Nu] * wv;
            sd += d * wv;
        }
    sn = col_sum(red[0], sn, fl, aj);
    sd = col_sum(red[1], sd, fl, aj);
    float sq = 0.f;
    if (act)
        for (int f = fl; f < F; f += CL) {
            const float n = num[(size_t)f * Nu], d = den[(size_t)f * Nu], wv = W[(size_t)f * N + n0 + j];
            const float wnew = wv * (n + sd * wv) / fmaxf(d + sn * wv, FLR);
            out[(size_t)f * Nu] = wnew;
            sq += wnew * wnew;
        }
    sq = col_sum(red[2], sq, fl, aj);
    const float nrm = sqrtf(sq);
    // a norm of 0 (a silent block: num and den are 0) or one that is not finite keeps the column as it was
    const bool ok = nrm > 0.f && nrm <= 3.4028234e38f;
    if (act)
        for (int f = fl; f < F; f += CL)
            out[(size_t)f * Nu] = ok ? out[(size_t)f * Nu] / nrm : W[(size_t)f * N + n0 + j];
}

// ... and the new columns into the dictionary
__global__ void __launch_bounds__(256)
snmf_online_commit_kernel(float* __restrict__ Wb, const float* __restrict__ Wt, const int* __restrict__ ph,
                          const int* __restrict__ nn, int s, int L, int F, int N, int n0) {
    const int b = blockIdx.y, Nu = N - n0, i = blockIdx.x * 256 + threadIdx.x;
    if (!block_full(ph, nn, b, s, L) || i >= F * Nu) return;
    const int f = i / Nu, j = i - f * Nu;
    Wb[((size_t)b * F + f) * N + n0 + j] = Wt[(size_t)b * F * Nu + i];
}

struct State {
    size_t off_count, off_W, off_A, off_Bm, off_V, off_H, total;
};
State state_layout(int B, int F, int N, int n0, int L) {
    State s;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += round_up_sz(bytes, 256); return at; };
    s.off_count = take((size_t)B * 8);
    s.off_W = take((size_t)B * F * N * 4);
    s.off_A = take((size_t)B * N * (N - n0) * 4);
    s.off_Bm = take((size_t)B * F * (N - n0) * 4);
    s.off_V = take((size_t)B * L * F * 4);
    s.off_H = take((size_t)B * L * N * 4);
    s.total = o;
    return s;
}

struct Work {
    size_t off_valid, off_pos, off_ph, off_n, off_todo, off_M, off_Wt, off_D, total;
};
Work work_layout(int B, int T, int F, int N, int n0, int L) {
    Work w;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += round_up_sz(bytes, 256); return at; };
    w.off_valid = take((size_t)B * T * 4);
    w.off_pos = take((size_t)B * T * 4);
    w.off_ph = take((size_t)B * 4);
    w.off_n = take((size_t)B * 4);
    w.off_todo = take((size_t)B * L * 4);
    w.off_M = take((size_t)B * L * F * 4);
    w.off_Wt = take((size_t)B * F * (N - n0) * 4);
    w.off_D = take((size_t)B * F * (N - n0) * 4);
    w.total = o;
    return w;
}

// A row of the state back to its start: W = Wn, everything else 0.  blockIdx.y: the row; rows: NULL or its flags.
__global__ void __launch_bounds__(256)
snmf_online_reset_kernel(const float* __restrict__ Wn, const int* __restrict__ rows, long long* __restrict__ count,
                         float* __restrict__ W, float* __restrict__ A, float* __restrict__ Bm,
                         float* __restrict__ Vblk, float* __restrict__ Hblk, int F, int N, int n0, int L) {
    const int b = blockIdx.y;
    if (rows && rows[b] == 0) return;
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    const size_t nW = (size_t)F * N, nA = (size_t)N * (N - n0), nB = (size_t)F * (N - n0), nV = (size_t)L * F,
                 nH = (size_t)L * N;
    if (i0 == 0) count[b] = 0;
    for (size_t i = i0; i < nW; i += step) W[b * nW + i] = Wn[i];
    for (size_t i = i0; i < nA; i += step) A[b * nA + i] = 0.f;
    for (size_t i = i0; i < nB; i += step) Bm[b * nB + i] = 0.f;
    for (size_t i = i0; i < nV; i += step) Vblk[b * nV + i] = 0.f;
    for (size_t i = i0; i < nH; i += step) Hblk[b * nH + i] = 0.f;
}

bool block_ok(int L) { return L >= MIN_BLOCK && L <= MAX_BLOCK && L % 16 == 0; }

bool shape_ok(int B, int F, int N, int n0, int L) {
    return B > 0 && B <= 65535 && F > 0 && N > 0 && N % 2 == 0 && n0 >= 0 && n0 <= N && block_ok(L);
}

// The checks reset, forward and read share: the shape, the state's size and alignment, the device
int32_t check_state(drnmf_handle_t h, const char* name, int B, int F, int N, int n0, int L, const void* state,
                    size_t state_bytes) {
    if (B <= 0 || F <= 0 || N <= 0) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: bad shape B=%d F=%d N=%d", name, B, F, N);
    if (N % 2) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: N = %d must be even (speech and noise halves)", name, N);
    if (n0 < 0 || n0 > N) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: n0 = %d fixed atoms of N = %d", name, n0, N);
    if (B > 65535) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: at most 65535 rows per call (B = %d)", name, B);
    if (!block_ok(L))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: block = %d must be a multiple of 16 in %d..%d", name, L, MIN_BLOCK,
                   MAX_BLOCK);
    if (!drnmf_snmf_online_admitted(F, N, 2.f, L))
        DRNMF_FAIL(h, DRNMF_ERR_UNSUPPORTED, "%s: the kernels take 2 <= N <= %d (N = %d)", name, MAX_N, N);
    const size_t need = state_layout(B, F, N, n0, L).total;
    if (!state || state_bytes < need || ((uintptr_t)state & 255))
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "%s: state of %zu bytes, required %zu (256-byte aligned)", name,
                   state ? state_bytes : (size_t)0, need);
    return DRNMF_OK;
}

struct Call {
    int device;
    hipStream_t stream;
    int B, T, F, N, n0, L, n_iter, w_iter;
    float sparsity, forget, power;
    const float *x, *h_init;
    float *mask_out, *H_out, *W, *A, *Bm, *Vblk, *Hblk, *Mst, *Wt, *D;
    int *pos, *ph, *nn, *todo;
};

template <int NTW, bool VEC>
hipError_t run_steps(const Call& c) {
    const int wide = widest_n(NTW), Nu = c.N - c.n0, S = (c.T + 2 * c.L - 2) / c.L;
    const dim3 slots((unsigned)c.L, (unsigned)c.B), tiles((unsigned)(c.L / TR), (unsigned)c.B);
    const dim3 sgrid((unsigned)((c.N + FC - 1) / FC + (c.F + FC - 1) / FC), (unsigned)c.B);
    auto stats_lds = [](int N) { return (size_t)(TR * (np16(N) + 8) + TR * LS) * sizeof(float); };
    hipError_t e;
    for (int s = 0; s < S; ++s) {
        hipLaunchKernelGGL(snmf_online_gather_kernel, slots, dim3(64), 0, c.stream, c.x, (const int*)c.pos,
                           (const int*)c.ph, (const int*)c.nn, c.todo, c.Vblk, s, c.T, c.F, c.L);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        e = launch_grid<snmf_online_h_kernel<NTW, VEC>>(c.device, lds_bytes(wide), lds_bytes(c.N), tiles, c.stream,
                                                        (const float*)c.Vblk, (const float*)c.W, c.h_init,
                                                        (const int*)c.todo, c.Hblk, c.Mst, c.L, c.F, c.N, c.n_iter,
                                                        c.sparsity, c.power);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(snmf_online_scatter_kernel, slots, dim3(64), 0, c.stream, (const int*)c.todo,
                           (const float*)c.Mst, (const float*)c.Hblk, c.mask_out, c.H_out, c.T, c.F, c.N, c.L);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (Nu == 0) continue;
        e = launch_grid<snmf_online_stats_kernel<NTW>>(c.device, stats_lds(wide), stats_lds(c.N), sgrid, c.stream,
                                                       (const float*)c.Vblk, (const float*)c.Hblk, c.A, c.Bm,
                                                       (const int*)c.ph, (const int*)c.nn, s, c.L, c.F, c.N, c.n0,
                                                       c.forget, c.power);
        if (e != hipSuccess) return e;
        for (int it = 0; it < c.w_iter; ++it) {
            hipLaunchKernelGGL(snmf_online_col_kernel, dim3((unsigned)((Nu + 15) / 16), (unsigned)c.B),
                               dim3(16 * CL), (size_t)c.N * 16 * sizeof(float), c.stream, (const float*)c.W,
                               (const float*)c.A, (const float*)c.Bm, c.Wt, c.D, (const int*)c.ph,
                               (const int*)c.nn, s, c.L, c.F, c.N, c.n0);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            hipLaunchKernelGGL(snmf_online_commit_kernel, dim3((unsigned)((c.F * Nu + 255) / 256), (unsigned)c.B),
                               dim3(256), 0, c.stream, c.W, (const float*)c.Wt, (const int*)c.ph, (const int*)c.nn,
                               s, c.L, c.F, c.N, c.n0);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace

extern "C" int32_t drnmf_snmf_online_admitted(int32_t F, int32_t N, float beta, int32_t block) {
    return (F > 0 && N >= 2 && N <= MAX_N && N % 2 == 0 && beta == 2.f && block_ok(block)) ? 1 : 0;
}

extern "C" size_t drnmf_snmf_online_state_bytes(int32_t B, int32_t F, int32_t N, int32_t n0, int32_t block) {
    if (!shape_ok(B, F, N, n0, block) || !drnmf_snmf_online_admitted(F, N, 2.f, block)) return 0;
    return state_layout(B, F, N, n0, block).total;
}

extern "C" size_t drnmf_snmf_online_workspace_bytes(int32_t B, int32_t T, int32_t F, int32_t N, int32_t n0,
                                                    int32_t block) {
    if (T <= 0 || !shape_ok(B, F, N, n0, block) || !drnmf_snmf_online_admitted(F, N, 2.f, block)) return 0;
    return work_layout(B, T, F, N, n0, block).total;
}

extern "C" int32_t drnmf_snmf_online_reset(drnmf_handle_t h, int32_t B, int32_t F, int32_t N, int32_t n0,
                                           int32_t block, const float* Wn, const int32_t* rows, void* state,
                                           size_t state_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (int32_t rc = check_pointers(h, "snmf_online_reset", {Wn})) return rc;
    if (int32_t rc = check_state(h, "snmf_online_reset", B, F, N, n0, block, state, state_bytes)) return rc;
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "snmf_online_reset: the handle is bound to no device");
    const State S = state_layout(B, F, N, n0, block);
    char* st = (char*)state;
    hipLaunchKernelGGL(snmf_online_reset_kernel, dim3(64, (unsigned)B), dim3(256), 0, (hipStream_t)stream_, Wn,
                       (const int*)rows, (long long*)(st + S.off_count), (float*)(st + S.off_W),
                       (float*)(st + S.off_A), (float*)(st + S.off_Bm), (float*)(st + S.off_V),
                       (float*)(st + S.off_H), F, N, n0, block);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

extern "C" int32_t drnmf_snmf_online_forward(drnmf_handle_t h, int32_t B, int32_t T, int32_t F, int32_t N,
                                             int32_t n0, int32_t block, int32_t n_iter, int32_t w_iter,
                                             float sparsity, float forget, float power, float mask_value,
                                             int32_t has_mask, const float* x, const float* h_init, float* mask_out,
                                             float* H_out, void* state, size_t state_bytes, void* workspace,
                                             size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    const char* name = "snmf_online_forward";
    if (int32_t rc = check_shape(h, name, B, T, F, N, n_iter)) return rc;
    if (w_iter < 0) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: w_iter = %d must not be negative", name, w_iter);
    if (!(forget > 0.f && forget <= 1.f))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: forget = %g must lie in (0, 1]", name, (double)forget);
    if (int32_t rc = check_flags(h, name, sparsity, has_mask)) return rc;
    if (int32_t rc = check_pointers(h, name, {x, h_init, mask_out})) return rc;
    if ((int64_t)B * T > 0x7fffff00)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: too many frames (%lld)", name, (long long)B * T);
    if (int32_t rc = check_state(h, name, B, F, N, n0, block, state, state_bytes)) return rc;
    const Work L = work_layout(B, T, F, N, n0, block);
    if (!workspace || workspace_bytes < L.total || ((uintptr_t)workspace & 255))
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "%s: workspace %zu < required %zu (256-byte aligned)", name,
                   workspace ? workspace_bytes : (size_t)0, L.total);
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "%s: the handle is bound to no device", name);
    const State S = state_layout(B, F, N, n0, block);
    char *st = (char*)state, *ws = (char*)workspace;
    Call c;
    c.device = h->device;
    c.stream = (hipStream_t)stream_;
    c.B = B, c.T = T, c.F = F, c.N = N, c.n0 = n0, c.L = block, c.n_iter = n_iter, c.w_iter = w_iter;
    c.sparsity = sparsity, c.forget = forget, c.power = power;
    c.x = x, c.h_init = h_init, c.mask_out = mask_out, c.H_out = H_out;
    c.W = (float*)(st + S.off_W), c.A = (float*)(st + S.off_A), c.Bm = (float*)(st + S.off_Bm);
    c.Vblk = (float*)(st + S.off_V), c.Hblk = (float*)(st + S.off_H);
    c.Mst = (float*)(ws + L.off_M), c.Wt = (float*)(ws + L.off_Wt), c.D = (float*)(ws + L.off_D);
    c.pos = (int*)(ws + L.off_pos), c.ph = (int*)(ws + L.off_ph), c.nn = (int*)(ws + L.off_n);
    c.todo = (int*)(ws + L.off_todo);
    int* valid = (int*)(ws + L.off_valid);
    hipLaunchKernelGGL(snmf_online_valid_kernel, dim3((unsigned)((T + 3) / 4), (unsigned)B), dim3(256), 0, c.stream, x,
                       valid, mask_out, H_out, T, F, N, mask_value, has_mask);
    DRNMF_HIP(h, hipGetLastError());
    hipLaunchKernelGGL(snmf_online_scan_kernel, dim3((unsigned)B), dim3(256), 0, c.stream, (const int*)valid, c.pos,
                       c.ph, c.nn, (long long*)(st + S.off_count), T, block);
    DRNMF_HIP(h, hipGetLastError());
    // (a row's dictionary starts 16-byte aligned when N % 4 == 0: the state is 256-byte aligned)
    const hipError_t e = with_instance(N, N % 4 == 0, [&](auto ntw, auto v) {
        return run_steps<decltype(ntw)::value, decltype(v)::value>(c);
    });
    DRNMF_HIP(h, e);
    return DRNMF_OK;
}

extern "C" int32_t drnmf_snmf_online_read(drnmf_handle_t h, int32_t B, int32_t F, int32_t N, int32_t n0,
                                          int32_t block, const void* state, size_t state_bytes, float* W_out,
                                          int64_t* counts_out, float* A_out, float* Bm_out, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (int32_t rc = check_state(h, "snmf_online_read", B, F, N, n0, block, state, state_bytes)) return rc;
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "snmf_online_read: the handle is bound to no device");
    const State S = state_layout(B, F, N, n0, block);
    const char* st = (const char*)state;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t Nu = (size_t)(N - n0);
    auto copy = [&](void* dst, size_t off, size_t bytes) {
        return (dst && bytes) ? hipMemcpyAsync(dst, st + off, bytes, hipMemcpyDeviceToDevice, stream) : hipSuccess;
    };
    DRNMF_HIP(h, copy(W_out, S.off_W, (size_t)B * F * N * 4));
    DRNMF_HIP(h, copy(counts_out, S.off_count, (size_t)B * 8));
    DRNMF_HIP(h, copy(A_out, S.off_A, (size_t)B * N * Nu * 4));
    DRNMF_HIP(h, copy(Bm_out, S.off_Bm, (size_t)B * F * Nu * 4));
    return DRNMF_OK;
}
