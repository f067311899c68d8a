// The sparse-NMF baseline's inference on fp16 matrix-core operands (include/drnmf_snmf_f16.h): the tile kernel of
// snmf_mask.hip -- a workgroup owns 16 frame rows for all n_iter iterations, the dictionary streams from L2
// through LDS 32 bins at a time, one staged chunk serves both products, nothing but x and the mask touches HBM --
// with the iteration's two products on v_mfma_f32_16x16x32_f16 (fp32 accumulation).  Per chunk c of FC = 32 bins
// (Wc = dict16[32 c .. 32 c + 31][:], _Float16, packed once by snmf_f16_pack_kernel):
//     Lambda_c = max(H16 Wc^T, flr)   16 x 32, contraction over the atoms in K-steps of 32: split over the four
//                                     waves by 32-atom blocks, the four fp32 partials added in wave order
//     den     += Lambda16_c Wc        16 x N, contraction over the chunk's 32 bins = ONE K-step per 16-column
//                                     tile; every wave owns the tiles w, w + 4, ... of den, num and H
// H16 = (_Float16)H is a shadow of the fp32 master H (registers), rewritten by the update
// H <- H * num / max(den + sparsity, flr); Lambda16 = (_Float16)Lambda.  num = V Wn (once) and the two products of
// the final mask run on the exact fp32 MFMA from the fp32 dictionary, as snmf_mask.hip's do.
//
// Per-row scale.  A valid row works on s V, s h_init, s sparsity, s flr and s 1e-9 with s = 2^-e,
// e = ceil(log2(max_f V[f])) (clamped to [-40, 100]; s = 1 for an all-zero row): algebraically the same iteration, exact
// in fp32, and V's largest bin lies in (1/2, 1] whatever the level of the frame.  The FIRST iteration's H is
// s h_init, which for a silent frame (s = 2^18) leaves fp16's range: its two products take t0 h_init and t0 flr
// with h_init's own scale t0 = 2^-ceil(log2 max h_init) (one number for every row), and den is multiplied by
// s / t0 afterwards (powers of two: exact).  From the second iteration on H follows V's level.
//
// Operand maps (common.h: slot (q, e) of A meets slot (q, e) of B):
//   first product   slot (q, e) of K-step S = atom 32 S + 8 q + e: A = 16 bytes of H16's row r, B = 16 bytes of
//                   the chunk's bin row r (r + 16 for the second 16 bins), both ds_read_b128.
//   second product  slot (q, e) = bin 16 (e >> 2) + 4 q + (e & 3): B comes TRANSPOSED out of the same [bin][atom]
//                   image, two ds_read_b64_tr_b16 per tile (16-lane group q gathers the [4 bins][16 atoms] block
//                   at bins 16 h + 4 q, lane 4 i + p of the group supplying bin row i, atoms 4 p .. 4 p + 3, and
//                   receives its own atom's four bins); A = two 16-byte reads per partial of the fp32 Lambda_c.
// A result element depends on its own A row and B column only and the k order on atom and bin indices only, so a
// row's mask is a function of that row, the dictionary and h_init: bit for bit, wherever the row sits.
//
// LDS.  fp16 rows (H16 [16][LDH], chunk [32][LDH]) have LDH = Np32 + 16 halves: a row stride of 32 bytes mod 64
// spreads every 16-lane group of the ds_read_b128 (rows 0-3, 12-15 at q and 4-11 at q + 1) over all sixteen
// 16-byte slots, and puts the eight bin rows of a 32-lane half of the transposing read (32 bytes each) on
// disjoint banks.  The fp32 partials have LLH = 40 floats per row for the same reason.  The fp32 phases in front
// of and behind the iterations are snmf_tile.h's, shared with the fp32 tile kernels: they use the same memory with the
// strides, the slot order and the bank reasoning written there.
#include "snmf_tile.h"

#include "../../include/drnmf_snmf_f16.h"

namespace {

using namespace snmf_tile;        // (FC = 32 bins is also one K-step of the second product here)

constexpr int LLH = 40;           // iterations: row stride of the fp32 partials of Lambda_c

inline int np32(int N) { return (N + 31) & ~31; }
// (the fp16 images fit inside the fp32 ones: 2 (Np32 + 16) <= 4 (Np16 + 8)); the tail: valid and the row scales
constexpr size_t f16_lds_bytes(int N) { return lds_bytes(N, LLH, 2 * TR); }
static_assert(f16_lds_bytes(200) == 51840 && f16_lds_bytes(MAX_N) == 110208, "as before the sizes were shared");

typedef __attribute__((__vector_size__(4 * sizeof(short)))) short s16x4;
typedef __attribute__((__vector_size__(8 * sizeof(short)))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// 2^-e with e = ceil(log2 m) clamped to [SCALE_E_MIN, SCALE_E_MAX]: m 2^-e lies in (1/2, 1] for m between 2^-40
// and 2^100.  1 for m = 0 (and for what is not a number).  The clamp keeps everything the scale multiplies inside
// its format: s <= 2^40 puts the scaled floor s 1e-9 at 1100 (finite in fp16; a frame below 2^-40 is under the
// floor anyway, its H goes to 0) and s h_init, s sparsity far from fp32's end; s >= 2^-100 keeps s h_init normal.
constexpr int SCALE_E_MIN = -40, SCALE_E_MAX = 100;
__device__ __forceinline__ float pow2_scale(float m) {
    if (!(m > 0.f && m <= 3.0e38f)) return 1.f;
    int e;
    const float fr = frexpf(m, &e);           // m = fr 2^e, fr in [1/2, 1): ceil(log2 m) = e, or e - 1 at fr = 1/2
    if (fr == 0.5f) --e;
    e = e < SCALE_E_MIN ? SCALE_E_MIN : (e > SCALE_E_MAX ? SCALE_E_MAX : e);
    return ldexpf(1.f, -e);
}
// fp32 -> fp16 operand, saturating at fp16's largest finite value: an operand is never inf, so a zero on the other
// side (the padding bins and atoms of a chunk) always gives a zero product
constexpr float F16_MAX = 65504.f;
__device__ __forceinline__ f16 to_f16_sat(float v) { return (f16)fminf(v, F16_MAX); }

// Wn [F][N] fp32 -> dict16 [F][Np32] _Float16, zero behind N
__global__ void __launch_bounds__(256)
snmf_f16_pack_kernel(const float* __restrict__ Wn, f16* __restrict__ dict16, int F, int N, int Np) {
    const int64_t total = (int64_t)F * Np;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int f = (int)(i / Np), c = (int)(i % Np);
        dict16[i] = c < N ? (f16)Wn[(size_t)f * N + c] : (f16)0.f;
    }
}

// NTW: 16-column tiles of H / num / den per wave (4: N <= 256, 8: N <= 512).  Waves per SIMD as snmf_mask.hip's.
template <int NTW>
__global__ void __launch_bounds__(256, NTW == 4 ? 3 : 1)
snmf_f16_tile_kernel(const float* __restrict__ x, const f16* __restrict__ dict16, const float* __restrict__ Wn,
                     const float* __restrict__ h_init, float* __restrict__ mask_out, int64_t rows, int F, int N,
                     int n_iter, float sparsity, float power, float mask_value, int has_mask) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Np = np16(N), NT = Np >> 4, LD = Np + 8, NC = (F + FC - 1) / FC;
    const int Nh = (N + 31) & ~31, NK = Nh >> 5, LDH = Nh + 16;
    float* Hs = smem;                         // [TR][LD]   fp32 H (final mask only)
    float* Ws = Hs + TR * LD;                 // [FC][LD]   fp32 dictionary chunk (numerator, final mask)
    f16* Hs16 = (f16*)Hs;                     // [TR][LDH]  the fp16 shadow of H        } the iterations, inside
    f16* Ws16 = (f16*)Ws;                     // [FC][LDH]  fp16 dictionary chunk       } the fp32 images
    float* Lp = Ws + FC * LD;                 // [4][TR][LLH] per-wave partials of Lambda_c; slot 0 also the V chunk
    int* valid = (int*)(Lp + 4 * TR * LLH);   // [TR]
    float* rs = (float*)(valid + TR);         // [TR] the row's scale s
    const int tid = threadIdx.x, l = tid & 63, r = l & 15, q = l >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * TR;
    const float flr = 1e-9f;                  // sparse_nmf_gpu.m:172

    // keras.layers.Masking (row_validity's rule) and the row's scale.  Not row_validity: the row's maximum rides on
    // the same read of x, has_mask or not, and is reduced beside __any
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rl = 4 * w + i;
        const int64_t row = row0 + rl;
        bool any = false;
        float m = 0.f;
        if (row < rows) {
            for (int f = l; f < F; f += 64) {
                const float xv = x[row * F + f];
                any |= (xv != mask_value);
                m = fmaxf(m, vpow(xv, power));    // (fmaxf drops a NaN)
            }
            if (!has_mask) any = true;
        }
        any = __any(any);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        const float s = pow2_scale(m);
        if (l == 0) {
            valid[rl] = any ? 1 : 0;
            rs[rl] = s;
        }
    }
    __syncthreads();
    if (all_masked(valid, mask_out, row0, rows, F, tid)) return;

    // the whole shadow once (the columns behind N and the rows that are not valid stay 0), ...
    for (int i = tid; i < TR * LDH / 2; i += 256) ((unsigned*)Hs16)[i] = 0u;
    __syncthreads();
    // ... then this lane's elements: rows 4 q + v, columns 16 t + r of its tiles t = w + 4 i
    // (h_init's own scale t0, for the first iteration's shadow: the same number in every lane and workgroup)
    float hmax = 0.f;
    for (int c = l; c < N; c += 64) hmax = fmaxf(hmax, h_init[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hmax = fmaxf(hmax, __shfl_xor(hmax, o));
    const float t0 = pow2_scale(hmax), inv_t0 = 1.f / t0;
    f32x4 num[NTW], den[NTW], Hm[NTW];
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const f32x4 sc = *(const f32x4*)(rs + 4 * q);
        const int t = w + 4 * i, col = 16 * t + r;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int rl = 4 * q + v;
            float hv = 0.f;
            if (t < NT && col < N && valid[rl]) hv = h_init[col];
            num[i][v] = 0.f;
            den[i][v] = 0.f;
            Hm[i][v] = hv * sc[v];
            if (t < NT) Hs16[rl * LDH + col] = to_f16_sat(hv * t0);        // the first iteration contracts t0 h_init
        }
    }

    // fp32 dictionary chunk (numerator and final mask: two passes over the dictionary in all, so no prefetch in
    // registers): global -> LDS, 8 bytes a piece (N is even).  Wave w stages the chunk's rows w, w + 4, ..
    constexpr int NVP = NTW / 2;
    auto stage = [&](int c) {
#pragma unroll
        for (int i = 0; i < FC / 4; ++i) {
            const int bin = c * FC + w + 4 * i;
#pragma unroll
            for (int p = 0; p < NVP; ++p) {
                const int col = 2 * (l + 64 * p);
                f32x2 v = {0.f, 0.f};
                if (bin < F && col < N) v = *(const f32x2*)(Wn + (size_t)bin * N + col);
                if (col < Np) *(f32x2*)(Ws + (w + 4 * i) * LD + col) = v;
            }
        }
    };
    // the fp16 chunk: global -> registers (in flight under the previous chunk's products) -> LDS, 16 bytes a piece.
    // A bin row of this instance is at most PPR = 8 NTW pieces (dict16 is zero behind N), so a wave's load takes
    // 64 / PPR rows at once: instruction i of wave w stages the rows (4 i + w) RPI ..
    constexpr int PPR = 8 * NTW, RPI = 64 / PPR;
    const int srow = l / PPR, scol = 8 * (l % PPR);
    f16x8 pf16[NTW];
    auto gload16 = [&](int c) {
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const int bin = c * FC + (4 * i + w) * RPI + srow;
            f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (bin < F && scol < Nh) v = *(const f16x8*)(dict16 + (size_t)bin * Nh + scol);
            pf16[i] = v;
        }
    };
    auto swrite16 = [&]() {
#pragma unroll
        for (int i = 0; i < NTW; ++i)
            if (scol < Nh) *(f16x8*)(Ws16 + ((4 * i + w) * RPI + srow) * LDH + scol) = pf16[i];
    };

    // num = (s V) Wn, once, exact fp32: V = x^power on valid rows, 0 elsewhere
    for (int c = 0; c < NC; ++c) {
        stage(c);
        num_fill(x, Lp, valid, rs, row0, F, c, power, tid);
        __syncthreads();
        num_accumulate<NTW>(Ws, Lp, LD, NT, w, r, q, num);
        __syncthreads();
    }

    // the iterations, on fp16 operands
    // transposing read of this lane: bin row 4 q + (r >> 2) of the 16-bin half, atoms 4 (r & 3) .. of the tile
    const f16* trp = Ws16 + (4 * q + (r >> 2)) * LDH + 4 * (r & 3);
    if (n_iter > 0) gload16(0);
    for (int it = 0; it < n_iter; ++it) {
        const float fl_a = (it == 0 ? t0 : rs[r]) * flr;      // the floor of Lambda at this lane's A row
#pragma unroll
        for (int i = 0; i < NTW; ++i) den[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < NC; ++c) {
            swrite16();
            __syncthreads();                  // the chunk (and, for c == 0, the new shadow) visible
            gload16(c + 1 < NC ? c + 1 : 0);
            f32x4 P[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int i = 0; i < NTW / 2; ++i) {
                const int S = w + 4 * i;
                if (S < NK) {
                    const int k0 = 32 * S + 8 * q;
                    const f16x8 a = *(const f16x8*)(Hs16 + r * LDH + k0);
                    const f16x8 b0 = *(const f16x8*)(Ws16 + r * LDH + k0);
                    const f16x8 b1 = *(const f16x8*)(Ws16 + (16 + r) * LDH + k0);
                    P[0] = mfma32h(a, b0, P[0]);
                    P[1] = mfma32h(a, b1, P[1]);
                }
            }
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                for (int v = 0; v < 4; ++v) Lp[(w * TR + 4 * q + v) * LLH + 16 * jt + r] = P[jt][v];
            __syncthreads();
            f16x8 a8;
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const float* p = Lp + r * LLH + 16 * hh + 4 * q;
                f32x4 sum = *(const f32x4*)p;                     // the four waves' partials, in wave order
                sum += *(const f32x4*)(p + TR * LLH);
                sum += *(const f32x4*)(p + 2 * TR * LLH);
                sum += *(const f32x4*)(p + 3 * TR * LLH);
#pragma unroll
                for (int e = 0; e < 4; ++e) a8[4 * hh + e] = to_f16_sat(fmaxf(sum[e], fl_a));
            }
#pragma unroll
            for (int i = 0; i < NTW; ++i) {
                const int t = w + 4 * i;
                if (t < NT) {                 // (wave-uniform: every lane takes part in the gather)
                    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(trp + 16 * t));
                    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(trp + 16 * LDH + 16 * t));
                    const f16x8 b = __builtin_bit_cast(f16x8, (s16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
                    den[i] = mfma32h(a8, b, den[i]);
                }
            }
            __syncthreads();                  // every wave is done with the chunk and Lp
        }
        const f32x4 sc = *(const f32x4*)(rs + 4 * q);         // (once per iteration: not worth four registers)
#pragma unroll
        for (int i = 0; i < NTW; ++i) {       // sparse_nmf_gpu.m:217-227 on the fp32 master
            const int t = w + 4 * i;
            if (t < NT) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float d = it == 0 ? den[i][v] * inv_t0 * sc[v] : den[i][v];
                    const float hn = Hm[i][v] * num[i][v] / fmaxf(d + sc[v] * sparsity, sc[v] * flr);
                    Hm[i][v] = hn;
                    Hs16[(4 * q + v) * LDH + 16 * t + r] = to_f16_sat(hn);
                }
            }
        }
    }
    __syncthreads();                          // the fp16 images are dead: fp32 H into the same memory

    // mask = Wc Hc / (s 1e-9 + Wc Hc + Wn Hn) from the fp32 master, a chunk at a time (enhance.py:848-852)
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int t = w + 4 * i;
        if (t < NT) {
#pragma unroll
            for (int v = 0; v < 4; ++v) Hs[(4 * q + v) * LD + 16 * t + r] = Hm[i][v];
        }
    }
    final_mask<NTW>(Hs, Ws, Lp, valid, rs, mask_out, row0, rows, F, N, LD, tid, w, r, q, [&](int c) {
        stage(c);
        __syncthreads();
    });
}

template <int NTW>
hipError_t launch_f16(const float* x, const f16* dict16, const float* Wn, const float* h_init, float* mask_out,
                      int64_t rows, int F, int N, int n_iter, float sparsity, float power, float mask_value,
                      int has_mask, hipStream_t stream, int device) {
    return launch<snmf_f16_tile_kernel<NTW>>(device, f16_lds_bytes(widest_n(NTW)), f16_lds_bytes(N), rows,
                                             stream, x, dict16, Wn, h_init, mask_out, rows, F, N, n_iter, sparsity,
                                             power, mask_value, has_mask);
}

}  // namespace

extern "C" int32_t drnmf_snmf_f16_admitted(int32_t F, int32_t N, float beta) {
    return (F > 0 && N >= 2 && N <= MAX_N && N % 2 == 0 && beta == 2.f) ? 1 : 0;
}

extern "C" size_t drnmf_snmf_f16_dict_bytes(int32_t F, int32_t N) {
    if (F <= 0 || N <= 0) return 0;
    return (size_t)F * np32(N) * sizeof(f16);
}

extern "C" int32_t drnmf_snmf_f16_pack_dict(drnmf_handle_t h, int32_t F, int32_t N, const float* Wn, void* dict16,
                                            size_t dict16_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (F <= 0 || N <= 0) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "snmf_f16_pack_dict: bad shape F=%d N=%d", F, N);
    if (!Wn || !dict16) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "snmf_f16_pack_dict: NULL pointer argument");
    if ((uintptr_t)dict16 & 15)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "snmf_f16_pack_dict: dict16 must be 16-byte aligned");
    const size_t need = drnmf_snmf_f16_dict_bytes(F, N);
    if (dict16_bytes < need)
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "snmf_f16_pack_dict: dict16 holds %zu bytes < required %zu", dict16_bytes,
                   need);
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "snmf_f16_pack_dict: the handle is bound to no device");
    const int Np = np32(N);
    const int64_t total = (int64_t)F * Np;
    const int64_t blocks = (total + 255) / 256;
    const unsigned grid = blocks > 4096 ? 4096u : (unsigned)blocks;
    hipLaunchKernelGGL(snmf_f16_pack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream_, Wn, (f16*)dict16, F, N,
                       Np);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

extern "C" int32_t drnmf_snmf_f16_forward(drnmf_handle_t h, int32_t B, int32_t T, int32_t F, int32_t N,
                                          int32_t n_iter, float sparsity, float power, float mask_value,
                                          int32_t has_mask, const float* x, const void* dict16, const float* Wn,
                                          const float* h_init, float* mask_out, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (int32_t rc = check_shape(h, "snmf_f16_forward", B, T, F, N, n_iter)) return rc;
    if (int32_t rc = check_flags(h, "snmf_f16_forward", sparsity, has_mask)) return rc;
    if (int32_t rc = check_pointers(h, "snmf_f16_forward", {x, dict16, Wn, h_init, mask_out})) return rc;
    if (((uintptr_t)dict16 & 15) || ((uintptr_t)Wn & 7))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "snmf_f16_forward: dict16 must be 16-byte and Wn 8-byte aligned");
    const int64_t rows = (int64_t)B * T;
    if (rows > 0x7fffff00)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "snmf_f16_forward: too many rows (%lld)", (long long)rows);
    if (N > MAX_N)
        DRNMF_FAIL(h, DRNMF_ERR_UNSUPPORTED, "snmf_f16_forward: the fp16 kernel takes N <= %d (N = %d)", MAX_N, N);
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "snmf_f16_forward: the handle is bound to no device");
    hipStream_t stream = (hipStream_t)stream_;
    const hipError_t e = np16(N) <= 256
        ? launch_f16<4>(x, (const f16*)dict16, Wn, h_init, mask_out, rows, F, N, n_iter, sparsity, power, mask_value,
                        has_mask, stream, h->device)
        : launch_f16<8>(x, (const f16*)dict16, Wn, h_init, mask_out, rows, F, N, n_iter, sparsity, power, mask_value,
                        has_mask, stream, h->device);
    DRNMF_HIP(h, e);
    return DRNMF_OK;
}
