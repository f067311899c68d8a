// LSTM baseline on gfx950: build_lstm (enhance.py:321-345), the paper's comparison model, inference path.
//
//     Masking(mask_value) -> LSTM(H, return_sequences=True) x K -> TimeDistributed(Dense(F))
//                         -> TimeDistributed(Activation('sigmoid'))
//
// Keras 2.0.4 LSTM [K2.0.4-memory]: z = x_t kernel + h_{t-1} recurrent_kernel + bias, gate columns i, f, c, o;
// i = s(z_i), f = s(z_f), c_t = f c_{t-1} + i tanh(z_c), o = s(z_o), h_t = o tanh(c_t), s = hard_sigmoid by
// default.  Masking as Theano's masked K.rnn (as cell_shared.h / cell_dense.hip): at a masked step the output
// and both states are the previous step's, in every layer.
//
// Launches of one forward:
//   1. pack:  x [B][T][F] -> xz [B*T][Fq] (masked frames zero, bins padded to a multiple of 4) + valid [B*T];
//   2. input projection of layer 0 for all B*T frames at once: xproj = xz . kernel_0 + bias_0 (gemm::launch,
//      bias in the epilogue; follows the handle's matrix mode like every frame-parallel product);
//   3. the recurrence as a WAVEFRONT over layers: layer k at frame t needs only (k-1, t) and (k, t-1), so one
//      launch per diagonal d = k + t runs every live (k, t) pair -- T + K - 1 launches instead of K T.  Layer
//      k >= 1 contracts the row block [h_{k-1,t} | h_{k,t-1}] with the stacked matrix [kernel_k; recurrent_k]
//      (the stacked-matrix idea of dense_step_kernel); layer 0 contracts h_{0,t-1} with recurrent_0 and adds
//      xproj[t].  Ordering comes from launch boundaries only: no workgroup waits on another.
// The head (sigmoid(h . W_out + b_out)) is one more gemm::launch with the sigmoid in its epilogue.
//
// operand_f16 (drnmf_lstm_desc_t, inference only): step 3 contracts fp16 operands on v_mfma_f32_16x16x32_f16 with
// fp32 accumulation.  The stacked matrices are STORED as _Float16 (lstm_pack_step_f16_kernel: the plain
// round-to-nearest cast params.hip uses for the cell's fp16 dictionary -- a weight beyond the fp16 range, |w| >
// 65504, becomes +-inf and poisons its gate column; nothing saturates or checks), and the h vectors entering the
// products come from an fp16 shadow of the h ring.  Everything else is as above in fp32: bias, xproj, the gates,
// c, the carried h, the final state, h_out, and steps 1, 2 and the head (which follow the matrix mode).
#include "common.h"
#include "gemm_nt.h"
#include "gemm_tn.h"
#include "../../include/drnmf_lstm.h"
#include "../../include/drnmf_waveloss.h"

namespace {

// Gate-interleaved packing of the 4H gate columns: output tile ab (32 columns) holds the gates i, f, c, o of
// the 8 units 8 ab .. 8 ab + 7, column 8 g + u = gate g of unit 8 ab + u.  The workgroup that contracts a tile
// then owns everything the cell update of its 16 rows x 8 units needs: c_t and h_t are formed from registers
// and LDS, no gate values go through memory.
constexpr int LSTM_UNITS = 8;
constexpr int LSTM_NW = 4;     // waves per workgroup (the contraction split over them, reduced through LDS)
constexpr int LSTM_G = 4;      // 16-row chunks in flight per wave
// 32-row fp16 chunks in flight per wave: 4 waves x 4 = 16 chunks = the whole contraction of H = 244 / 250
// (Hc = 256, layers k >= 1) in ONE round trip of 12 16-byte loads per lane, the same number the fp32 path keeps in
// flight.  Smaller H leaves slots over (H = 54: 2 or 4 chunks, H = 70: 3 or 6): they re-read the last valid chunk
// (the same cache lines) with a zeroed A term.
constexpr int LSTM_GH = 4;

struct LstmLayout {
    int Bp, Hc, Hq, Fq, numU, NC;
    bool half;                 // operand_f16: stacked matrices stored as _Float16, Hc a multiple of 32, h16 ring
    size_t off_bias, off_k0t, off_wo, off_bo, params_total;
    size_t off_xz, off_valid, off_xproj, off_h, off_c, off_h16, off_ctr, ws_total;
    // elements (floats, or halves with operand_f16) before layer k's stacked matrix: layer 0 has Hc rows
    // (recurrent_0), layers k >= 1 have 2 Hc
    size_t m_elems(int k) const { return k == 0 ? 0 : (size_t)Hc * NC * (2 * k - 1); }
};

LstmLayout lstm_layout(const drnmf_lstm_desc_t* d) {
    LstmLayout L;
    L.Bp = pad_b(d->B > 0 ? d->B : 1);
    L.half = d->operand_f16 == 1;
    // activation width: whole chunks of the contraction (16 rows per v_mfma_f32_16x16x4_f32 group, 32 per
    // v_mfma_f32_16x16x32_f16), so that each half of [h_{k-1,t} | h_{k,t-1}] is whole chunks
    L.Hc = round_up(d->H, L.half ? 32 : 16);
    L.Hq = round_up(d->H, 4);
    L.Fq = round_up(d->F, 4);              // xz / kernel_0^T rows: 16-byte loads in the gemm
    L.numU = (d->H + LSTM_UNITS - 1) / LSTM_UNITS;
    L.NC = L.numU * 32;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += round_up_sz(bytes, 256); return at; };
    take(L.m_elems(d->K) * (L.half ? 2 : 4));
    L.off_bias = take((size_t)d->K * L.NC * 4);
    L.off_k0t = take((size_t)L.NC * L.Fq * 4);
    L.off_wo = take((size_t)d->F * L.Hq * 4);
    L.off_bo = take((size_t)d->F * 4);
    L.params_total = o;
    o = 0;
    const size_t rows = (size_t)(d->B > 0 ? d->B : 0) * (d->T > 0 ? d->T : 0);
    L.off_xz = take(rows * L.Fq * 4);
    L.off_valid = take(rows);
    L.off_xproj = take(rows * L.NC * 4);
    L.off_h = take((size_t)d->K * 2 * L.Bp * L.Hc * 4);
    L.off_c = take((size_t)d->K * 2 * L.Bp * L.Hc * 4);
    L.off_h16 = L.half ? take((size_t)d->K * 2 * L.Bp * L.Hc * 2) : 0;     // fp16 shadow of the h ring
    L.off_ctr = take(256);
    L.ws_total = o;
    return L;
}

int validate_lstm_desc(drnmf_handle_t h, const drnmf_lstm_desc_t* d, bool need_bt) {
    if (!d) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "lstm desc is NULL");
    if ((need_bt && (d->B <= 0 || d->T <= 0)) || d->F <= 0 || d->H <= 0 || d->K <= 0)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "B,T,F,H,K must be positive (got %d,%d,%d,%d,%d)",
                   d->B, d->T, d->F, d->H, d->K);
    if (d->recurrent_activation != DRNMF_ACT_HARD_SIGMOID && d->recurrent_activation != DRNMF_ACT_SIGMOID)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG,
                   "recurrent_activation must be DRNMF_ACT_HARD_SIGMOID or DRNMF_ACT_SIGMOID (got %d)",
                   d->recurrent_activation);
    if (d->operand_f16 != 0 && d->operand_f16 != 1)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "operand_f16 must be 0 or 1 (got %d)", d->operand_f16);
    if (d->H > 8192 || d->F > 65536 || d->K > 1024)
        DRNMF_FAIL(h, DRNMF_ERR_UNSUPPORTED, "lstm: H <= 8192, F <= 65536, K <= 1024 (got %d, %d, %d)",
                   d->H, d->F, d->K);
    if (need_bt) {
        const int64_t rows = (int64_t)d->B * d->T;
        const int64_t widest = (d->F > 4 * d->H ? (int64_t)d->F : 4 * (int64_t)d->H) + 32;
        if (rows > 0x7fffff00 || rows * widest >= (1ll << 40))
            DRNMF_FAIL(h, DRNMF_ERR_UNSUPPORTED, "lstm: B*T too large");
    }
    return DRNMF_OK;
}

__device__ __forceinline__ float gate_act(float v, int act) {
    return act == DRNMF_ACT_SIGMOID ? 1.f / (1.f + expf(-v)) : fminf(fmaxf(0.2f * v + 0.5f, 0.f), 1.f);
}

// ---- parameter packing -------------------------------------------------------------------------------------

// Stacked matrix of layer k in the operand order of lstm_step_kernel: 16-row chunk c, output tile ab -> one
// block of 512 floats, two halves of 256 (packed columns 0..15 / 16..31 of the tile); lane (q, j) of a half
// holds rows 16 c + 4 q + s, s = 0..3, of column j as one 16-byte piece.  Rows: layer 0 = recurrent_0 [Hc];
// layer k >= 1 = kernel_k [Hc] then recurrent_k [Hc].  Padded rows / units are zero.
__global__ void __launch_bounds__(256)
lstm_pack_step_kernel(const float* __restrict__ kern, const float* __restrict__ rec, float* __restrict__ M,
                      int H, int Hc, int numU, int L) {
    const int NC = numU * 32;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)L * NC) return;
    const int i = (int)(idx / NC), p = (int)(idx % NC);
    const int g = (p & 31) >> 3, unit = (p >> 5) * LSTM_UNITS + (p & 7);
    float v = 0.f;
    if (unit < H) {
        const float* src = kern ? (i < Hc ? kern : rec) : rec;
        const int r = kern && i >= Hc ? i - Hc : i;
        if (r < H) v = src[(size_t)r * 4 * H + (size_t)g * H + unit];
    }
    const int c = i >> 4, kk = i & 15, q = kk >> 2, s = kk & 3;
    const int ab = p >> 5, pc = p & 31;
    M[((size_t)c * numU + ab) * 512 + (pc >> 4) * 256 + (q * 16 + (pc & 15)) * 4 + s] = v;
}

// The same matrix for the fp16 step kernel (operand_f16), in the operand order of mfma32h: 32-row chunk c, output
// tile ab -> one block of 1024 halves, two halves of 512 (packed columns 0..15 / 16..31 of the tile); lane (q, j) of
// a half holds rows 32 c + 8 q + e, e = 0..7, of column j as one 16-byte piece.  Hc is a multiple of 32 here.
// Plain round-to-nearest cast (as params.hip's fp16 dictionary): |w| > 65504 becomes +-inf.
__global__ void __launch_bounds__(256)
lstm_pack_step_f16_kernel(const float* __restrict__ kern, const float* __restrict__ rec, f16* __restrict__ M,
                          int H, int Hc, int numU, int L) {
    const int NC = numU * 32;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)L * NC) return;
    const int i = (int)(idx / NC), p = (int)(idx % NC);
    const int g = (p & 31) >> 3, unit = (p >> 5) * LSTM_UNITS + (p & 7);
    float v = 0.f;
    if (unit < H) {
        const float* src = kern ? (i < Hc ? kern : rec) : rec;
        const int r = kern && i >= Hc ? i - Hc : i;
        if (r < H) v = src[(size_t)r * 4 * H + (size_t)g * H + unit];
    }
    const int c = i >> 5, kk = i & 31, q = kk >> 3, e = kk & 7;
    const int ab = p >> 5, pc = p & 31;
    M[((size_t)c * numU + ab) * 1024 + (pc >> 4) * 512 + (q * 16 + (pc & 15)) * 8 + e] = (f16)v;
}

// bias [K][4H] -> [K][NC] in the packed column order
__global__ void __launch_bounds__(256)
lstm_pack_bias_kernel(const float* __restrict__ b, float* __restrict__ out, int H, int NC, int K) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K * NC) return;
    const int k = i / NC, p = i % NC;
    const int g = (p & 31) >> 3, unit = (p >> 5) * LSTM_UNITS + (p & 7);
    out[i] = unit < H ? b[(size_t)k * 4 * H + (size_t)g * H + unit] : 0.f;
}

// kernel_0 [F][4H] -> the "Bt" of the input projection, [NC][Fq] (K contiguous), packed column order
__global__ void __launch_bounds__(256)
lstm_pack_k0t_kernel(const float* __restrict__ k0, float* __restrict__ out, int F, int Fq, int H, int NC) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)NC * Fq) return;
    const int p = (int)(i / Fq), f = (int)(i % Fq);
    const int g = (p & 31) >> 3, unit = (p >> 5) * LSTM_UNITS + (p & 7);
    out[i] = (unit < H && f < F) ? k0[(size_t)f * 4 * H + (size_t)g * H + unit] : 0.f;
}

// w_out [H][F] -> [F][Hq] (the head's "Bt")
__global__ void __launch_bounds__(256)
lstm_pack_wo_kernel(const float* __restrict__ wo, float* __restrict__ out, int F, int H, int Hq) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)F * Hq) return;
    const int f = (int)(i / Hq), k = (int)(i % Hq);
    out[i] = k < H ? wo[(size_t)k * F + f] : 0.f;
}

// ---- forward -----------------------------------------------------------------------------------------------

// x [rows][F] -> xz [rows][Fq] and valid [rows]: one wave per frame.  [K2.0.4-memory: keras.layers.Masking --
// a frame is masked when every bin equals mask_value; its input is zeroed]
__global__ void __launch_bounds__(256)
lstm_pack_x_kernel(const float* __restrict__ x, float* __restrict__ xz, unsigned char* __restrict__ valid,
                   float mask_value, size_t rows, int F, int Fq) {
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + wv;
    if (row >= rows) return;
    const float* src = x + row * F;
    bool any = false;
    for (int f = l; f < F; f += 64) any |= (src[f] != mask_value);
    any = __any(any);
    float* dst = xz + row * Fq;
    for (int f = l; f < Fq; f += 64) dst[f] = (any && f < F) ? src[f] : 0.f;
    if (l == 0) valid[row] = any ? 1 : 0;
}

// zero initial h and c of every layer (both ring slots, padding included; h16: the fp16 shadow of the h ring,
// NULL without operand_f16), diagonal counters = 0
__global__ void __launch_bounds__(256)
lstm_init_kernel(float* __restrict__ hring, float* __restrict__ cring, f16* __restrict__ h16, int* ctr, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) { ctr[0] = 0; ctr[16] = 0; }
    if (i < n) {
        hring[i] = 0.f;
        cring[i] = 0.f;
        if (h16) h16[i] = (f16)0.f;
    }
}

// The *_stateful entry points: caller-owned state arrays [K][B][H]; NULL initial = zeros, NULL final = not wanted
struct LstmState {
    const float* initial_h;
    const float* initial_c;
    float* final_h;
    float* final_c;
};

// lstm_init_kernel with an entering state: frame 0 of layer k reads ring slot (-1) & 1 = 1, so the state
// [K][B][H] goes there (rows b < B, units n < H); the padded rows B .. Bp-1, the padded units H .. Hc-1 and all of
// slot 0 are zeros, diagonal counters = 0.  h16 (NULL without operand_f16): the fp16 shadow of the h ring, the same
// elements rounded.  Runs before the replayed frames, outside them.
__global__ void __launch_bounds__(256)
lstm_state_scatter_kernel(float* __restrict__ hring, float* __restrict__ cring, f16* __restrict__ h16, int* ctr,
                          const float* __restrict__ init_h, const float* __restrict__ init_c, size_t n, int B,
                          int H, int Bp, int Hc) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) { ctr[0] = 0; ctr[16] = 0; }
    if (i >= n) return;
    const size_t slab = (size_t)Bp * Hc;
    const size_t ks = i / slab, e = i % slab;            // ks = 2 k + slot
    const int b = (int)(e / Hc), u = (int)(e % Hc);
    float hv = 0.f, cv = 0.f;
    if ((ks & 1) && b < B && u < H) {
        const size_t s = ((ks >> 1) * B + b) * H + u;
        if (init_h) hv = init_h[s];
        if (init_c) cv = init_c[s];
    }
    hring[i] = hv;
    cring[i] = cv;
    if (h16) h16[i] = (f16)hv;
}

// the state leaving the call: ring slot (T - 1) & 1 of every layer -> final_h / final_c [K][B][H] (either may be
// NULL).  Runs behind the last replayed frame, outside the graphs.
__global__ void __launch_bounds__(256)
lstm_state_gather_kernel(const float* __restrict__ hring, const float* __restrict__ cring,
                         float* __restrict__ fin_h, float* __restrict__ fin_c, size_t n, int B, int H, int Bp,
                         int Hc, int slot) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t k = i / ((size_t)B * H), e = i % ((size_t)B * H);
    const size_t b = e / H, u = e % H;
    const size_t s = ((k * 2 + slot) * Bp + b) * Hc + u;
    if (fin_h) fin_h[i] = hring[s];
    if (fin_c) fin_c[i] = cring[s];
}

// training layout: the entering state into row b (T + 1) of every layer's stash (behind lstm_stash_init_kernel's
// zero fill), h into hst and c into cst; valid stays 0 there and z zero.  The BPTT reads c_{t-1} at t = 0 from
// this row, and the recurrent-kernel product its h.
__global__ void __launch_bounds__(256)
lstm_stash_state_kernel(float* __restrict__ cst, float* __restrict__ hst, const float* __restrict__ init_h,
                        const float* __restrict__ init_c, size_t n, int B, int H, int T, size_t RS, int Hc,
                        int Hq) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t k = i / ((size_t)B * H), e = i % ((size_t)B * H);
    const size_t b = e / H, u = e % H;
    const size_t srow = k * RS + b * ((size_t)T + 1);
    if (init_h) hst[srow * Hq + u] = init_h[i];
    if (init_c) cst[srow * Hc + u] = init_c[i];
}

struct EpiLstmXproj {   // xproj = acc + bias_0 (packed columns)
    float* out;
    const float* bias;
    int ldc;
    __device__ f32x2 pre(int64_t, int col) const { return f32x2{bias[col], 0.f}; }
    __device__ void operator()(int64_t row, int col, float acc, f32x2 p) const {
        out[row * ldc + col] = acc + p[0];
    }
};

struct EpiLstmHead {    // out = sigmoid(acc + b_out)
    float* out;
    const float* b;
    int F;
    __device__ f32x2 pre(int64_t, int col) const { return f32x2{b[col], 0.f}; }
    __device__ void operator()(int64_t row, int col, float acc, f32x2 p) const {
        out[row * F + col] = 1.f / (1.f + expf(-(acc + p[0])));
    }
};

struct LstmStepArgs {
    const float* M;            // every layer's stacked matrix (lstm_pack_step_kernel), layer k at m_floats(k)
    const float* bias;         // [K][NC] packed (layer 0's enters through xproj)
    const float* xproj;        // [B*T][NC]
    const unsigned char* valid;   // [B*T]
    float* hring;              // [K][2][Bp][Hc]: h_{k,t} in slot t & 1
    float* cring;              // [K][2][Bp][Hc]
    float* out;                // [B][T][ld_h]: the last layer's outputs, zeros in columns H .. ld_h-1
    const int* d_rd;           // diagonal counter read by every workgroup ...
    int* d_wr;                 // ... and the other one, advanced by workgroup (0, 0, 0)
    int B, T, H, K, Bp, Hc, numU, NC, act, ld_h;
    // training forward only (lstm_step_kernel<true>): xproj / valid in the training layout (row b (T+1) + t + 1)
    // and the stash of every (layer, frame): gate pre-activations, c_t and h_t at that row of layer k's block
    float* zst;                // [K][zk][NC]   packed columns
    float* cst;                // [K][Bp (T+1)][Hc]
    float* hst;                // [K][Bp (T+1)][Hq]
    size_t zk;                 // rows of one layer's block of zst (Bp (T+1) + 1: a zero row behind the last)
    int Hq;
    // operand_f16 only (lstm_step_kernel<false, true>): M then holds _Float16 (lstm_pack_step_f16_kernel)
    f16* h16;                  // [K][2][Bp][Hc]: (_Float16)h_{k,t} in slot t & 1, the A operand of the products
};

// One launch = one diagonal d: workgroup (ab, mb, k) computes frame t = d - k of layer k for rows
// 16 mb .. 16 mb + 15 and units 8 ab .. 8 ab + 7 (exits at once when t is out of range).  Exact-fp32 MFMA
// (v_mfma_f32_16x16x4_f32) over the contraction, split over the waves and reduced through LDS as in
// dense_step_kernel; the activations are read row-major -- lane (q, row j) takes h[j][16 c + 4 q .. + 3] as one
// 16-byte piece, which is the order the matrix packing puts the rows in.  Ring slots: (k, t) writes slot
// t & 1 of layer k; in the same launch (k + 1, t - 1) and (k, t) read slot (t - 1) & 1 of layer k, and (k, t)
// reads slot t & 1 of layer k - 1, which (k - 1, t + 1) does not write (it writes slot (t + 1) & 1).
// STASH (the training forward): the same arithmetic, plus the stash writes; lstm_step_kernel<false, false> is the
// inference kernel.
// HALF (operand_f16, inference only): the contraction runs on v_mfma_f32_16x16x32_f16, two per 32-row chunk, fp32
// accumulation; lane (q, row j) takes h16[j][32 c + 8 q .. + 7] from the fp16 shadow ring as one 16-byte piece and
// two 16-byte pieces of the fp16 packed block.  The cell update is the fp32 one on the fp32 rings (a masked step
// carries the fp32 h, the final state and h_out are fp32) and ALSO writes (_Float16)h_t into the shadow: the
// copy at a masked step, zero for a padded unit.  The shadow's slots are the fp32 ring's, written by the same
// thread in the same launch, so the reasoning above holds for it word for word: (k, t) writes shadow slot t & 1
// of layer k; in the same launch (k + 1, t - 1) and (k, t) read shadow slot (t - 1) & 1 of layer k, and (k, t)
// reads shadow slot t & 1 of layer k - 1, which (k - 1, t + 1) does not write.
template <bool STASH, bool HALF>
__global__ void __launch_bounds__(64 * LSTM_NW) lstm_step_kernel(const LstmStepArgs a) {
    static_assert(!(STASH && HALF), "operand_f16 is inference only");
    __shared__ __attribute__((aligned(16))) float red[LSTM_NW * 16 * 32];
    const int ab = blockIdx.x, mb = blockIdx.y, k = blockIdx.z;
    const int d = *a.d_rd;
    if (ab == 0 && mb == 0 && k == 0 && threadIdx.x == 0) *a.d_wr = d + 1;
    const int t = d - k;
    if (t < 0 || t >= a.T) return;
    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63, j = l & 15, q = l >> 4;
    const int Hc = a.Hc;
    const size_t slab = (size_t)a.Bp * Hc;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    if constexpr (HALF) {
        const int nh = Hc / 32, nch = k == 0 ? nh : 2 * nh;
        const size_t arow = (size_t)(mb * 16 + j) * Hc + 8 * q;
        const f16* prev = a.h16 + ((size_t)k * 2 + ((t + 1) & 1)) * slab + arow;                    // h_{k,t-1}
        const f16* below = k > 0 ? a.h16 + ((size_t)(k - 1) * 2 + (t & 1)) * slab + arow : prev;     // h_{k-1,t}
        const size_t m_off = k == 0 ? 0 : (size_t)Hc * a.NC * (2 * k - 1);
        const f16* brow = (const f16*)a.M + m_off + (size_t)ab * 1024 + l * 8;
        const size_t bstep = (size_t)a.numU * 1024;
        const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int c0 = w; c0 < nch; c0 += LSTM_NW * LSTM_GH) {
            f16x8 av[LSTM_GH], b0[LSTM_GH], b1[LSTM_GH];
#pragma unroll
            for (int g = 0; g < LSTM_GH; ++g) {
                const int c = c0 + LSTM_NW * g;
                const int cc = c < nch ? c : nch - 1;       // (clamped: a valid address, the term zeroed below)
                const f16* ap = k == 0 ? prev + 32 * cc : (cc < nh ? below + 32 * cc : prev + 32 * (cc - nh));
                av[g] = *(const f16x8*)ap;
                b0[g] = *(const f16x8*)(brow + (size_t)cc * bstep);
                b1[g] = *(const f16x8*)(brow + (size_t)cc * bstep + 512);
                if (c >= nch) av[g] = zero8;
            }
#pragma unroll
            for (int g = 0; g < LSTM_GH; ++g) {
                acc0 = mfma32h(av[g], b0[g], acc0);
                acc1 = mfma32h(av[g], b1[g], acc1);
            }
        }
    } else {
        const int nh = Hc / 16, nch = k == 0 ? nh : 2 * nh;
        const size_t arow = (size_t)(mb * 16 + j) * Hc + 4 * q;
        const float* prev = a.hring + ((size_t)k * 2 + ((t + 1) & 1)) * slab + arow;                 // h_{k,t-1}
        const float* below = k > 0 ? a.hring + ((size_t)(k - 1) * 2 + (t & 1)) * slab + arow : prev;  // h_{k-1,t}
        const size_t m_off = k == 0 ? 0 : (size_t)Hc * a.NC * (2 * k - 1);
        const float* brow = a.M + m_off + (size_t)ab * 512 + l * 4;
        const size_t bstep = (size_t)a.numU * 512;
        for (int c0 = w; c0 < nch; c0 += LSTM_NW * LSTM_G) {
            f32x4 av[LSTM_G], b0[LSTM_G], b1[LSTM_G];
#pragma unroll
            for (int g = 0; g < LSTM_G; ++g) {
                const int c = c0 + LSTM_NW * g;
                const int cc = c < nch ? c : nch - 1;       // (clamped: a valid address, the term zeroed below)
                const float* ap = k == 0 ? prev + 16 * cc : (cc < nh ? below + 16 * cc : prev + 16 * (cc - nh));
                av[g] = *(const f32x4*)ap;
                b0[g] = *(const f32x4*)(brow + (size_t)cc * bstep);
                b1[g] = *(const f32x4*)(brow + (size_t)cc * bstep + 256);
                if (c >= nch) av[g] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int g = 0; g < LSTM_G; ++g)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    acc0 = mfma16(av[g][s], b0[g][s], acc0);
                    acc1 = mfma16(av[g][s], b1[g][s], acc1);
                }
        }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        red[(w * 16 + 4 * q + v) * 32 + j] = acc0[v];
        red[(w * 16 + 4 * q + v) * 32 + 16 + j] = acc1[v];
    }
    __syncthreads();
    if (tid >= 16 * LSTM_UNITS) return;

    // cell update: thread = (row r, unit u) of the tile
    const int r = tid >> 3, u = tid & 7;
    const int b = mb * 16 + r, n = ab * LSTM_UNITS + u;
    const size_t frame = (size_t)b * a.T + t;
    const size_t frame_x = STASH ? (size_t)b * (a.T + 1) + t + 1 : frame;
    const bool real = b < a.B;
    if (n >= a.H) {                                     // padded units stay zero (they meet zero matrix rows)
        if (k == a.K - 1 && real && n < a.ld_h) a.out[frame * a.ld_h + n] = 0.f;
        if constexpr (HALF) a.h16[((size_t)k * 2 + (t & 1)) * slab + (size_t)b * Hc + n] = (f16)0.f;
        if constexpr (STASH) {
            const size_t srow = (size_t)k * a.Bp * (a.T + 1) + (size_t)b * (a.T + 1) + t + 1;
            float* zp = a.zst + ((size_t)k * a.zk + (size_t)b * (a.T + 1) + t + 1) * a.NC + ab * 32 + u;
#pragma unroll
            for (int g = 0; g < 4; ++g) zp[g * 8] = 0.f;
            a.cst[srow * a.Hc + n] = 0.f;
            if (n < a.Hq) a.hst[srow * a.Hq + n] = 0.f;
        }
        return;
    }
    const float* pre = k == 0 ? a.xproj + (real ? frame_x : 0) * a.NC : a.bias + (size_t)k * a.NC;
    float z[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float s = 0.f;
#pragma unroll
        for (int ww = 0; ww < LSTM_NW; ++ww) s += red[(ww * 16 + r) * 32 + g * 8 + u];
        z[g] = s + pre[ab * 32 + g * 8 + u];
    }
    const size_t e_prev = ((size_t)k * 2 + ((t + 1) & 1)) * slab + (size_t)b * Hc + n;
    const size_t e_cur = ((size_t)k * 2 + (t & 1)) * slab + (size_t)b * Hc + n;
    float cn = a.cring[e_prev], hn = a.hring[e_prev];   // K.rnn masking: a masked step keeps both states
    if (real && a.valid[frame_x]) {
        const float ig = gate_act(z[0], a.act), fg = gate_act(z[1], a.act), og = gate_act(z[3], a.act);
        cn = fg * cn + ig * tanhf(z[2]);
        hn = og * tanhf(cn);
    }
    a.cring[e_cur] = cn;
    a.hring[e_cur] = hn;
    if constexpr (HALF) a.h16[e_cur] = (f16)hn;
    if (k == a.K - 1 && real) a.out[frame * a.ld_h + n] = hn;
    if constexpr (STASH) {
        const size_t srow = (size_t)k * a.Bp * (a.T + 1) + (size_t)b * (a.T + 1) + t + 1;
        float* zp = a.zst + ((size_t)k * a.zk + (size_t)b * (a.T + 1) + t + 1) * a.NC + ab * 32 + u;
#pragma unroll
        for (int g = 0; g < 4; ++g) zp[g * 8] = z[g];
        a.cst[srow * a.Hc + n] = cn;
        a.hst[srow * a.Hq + n] = hn;
    }
}

}  // namespace

extern "C" size_t drnmf_lstm_params_bytes(const drnmf_lstm_desc_t* d) {
    if (!d || d->F <= 0 || d->H <= 0 || d->K <= 0) return 0;
    return lstm_layout(d).params_total;
}

extern "C" size_t drnmf_lstm_workspace_bytes(const drnmf_lstm_desc_t* d) {
    if (!d || d->B <= 0 || d->T <= 0 || d->F <= 0 || d->H <= 0 || d->K <= 0) return 0;
    return lstm_layout(d).ws_total;
}

extern "C" int32_t drnmf_lstm_prepare_params(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* kernel0,
                                             const float* kernel_rest, const float* recurrent,
                                             const float* bias, const float* w_out, const float* b_out,
                                             void* params, size_t params_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    int rc = validate_lstm_desc(h, d, false);
    if (rc) return rc;
    if (!kernel0 || !recurrent || !bias || !w_out || !b_out || !params || (d->K > 1 && !kernel_rest))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "lstm_prepare_params: NULL pointer argument");
    if ((uintptr_t)params & 255) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "params must be 256-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const LstmLayout L = lstm_layout(d);
    if (params_bytes < L.params_total)
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "lstm_prepare_params: params %zu < required %zu", params_bytes,
                   L.params_total);
    char* base = (char*)params;
    const size_t HH4 = (size_t)d->H * 4 * d->H;
    for (int k = 0; k < d->K; ++k) {
        const int rows = k == 0 ? L.Hc : 2 * L.Hc;
        const size_t tot = (size_t)rows * L.NC;
        const float* kern = k == 0 ? nullptr : kernel_rest + (size_t)(k - 1) * HH4;
        if (L.half)
            hipLaunchKernelGGL(lstm_pack_step_f16_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream,
                               kern, recurrent + (size_t)k * HH4, (f16*)base + L.m_elems(k), d->H, L.Hc, L.numU,
                               rows);
        else
            hipLaunchKernelGGL(lstm_pack_step_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream,
                               kern, recurrent + (size_t)k * HH4, (float*)base + L.m_elems(k), d->H, L.Hc, L.numU,
                               rows);
    }
    hipLaunchKernelGGL(lstm_pack_bias_kernel, dim3((unsigned)((d->K * L.NC + 255) / 256)), dim3(256), 0, stream,
                       bias, (float*)(base + L.off_bias), d->H, L.NC, d->K);
    const size_t nk = (size_t)L.NC * L.Fq, nw = (size_t)d->F * L.Hq;
    hipLaunchKernelGGL(lstm_pack_k0t_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, stream, kernel0,
                       (float*)(base + L.off_k0t), d->F, L.Fq, d->H, L.NC);
    hipLaunchKernelGGL(lstm_pack_wo_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, stream, w_out,
                       (float*)(base + L.off_wo), d->F, d->H, L.Hq);
    DRNMF_HIP(h, hipGetLastError());
    DRNMF_HIP(h, hipMemcpyAsync(base + L.off_bo, b_out, (size_t)d->F * 4, hipMemcpyDeviceToDevice, stream));
    return DRNMF_OK;
}

// final_h / final_c of a stateful call (nothing to do for st == nullptr or when neither is wanted)
static int32_t lstm_store_state(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const LstmLayout& L,
                                const float* hring, const float* cring, const LstmState* st, hipStream_t stream) {
    if (!st || (!st->final_h && !st->final_c)) return DRNMF_OK;
    const size_t n = (size_t)d->K * d->B * d->H;
    hipLaunchKernelGGL(lstm_state_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, hring,
                       cring, st->final_h, st->final_c, n, d->B, d->H, L.Bp, L.Hc, (d->T - 1) & 1);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

// Row stride, then params alignment: the order of the head, the loss head and the training forwards (the inference
// forwards check the workspace size between the two and have one alignment message for workspace and params)
static int32_t lstm_check_ld_params(drnmf_handle_t h, const drnmf_lstm_desc_t* d, int32_t ld_h, const void* params,
                                    const char* what) {
    if (ld_h < d->H) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: ld_h %d < H %d", what, ld_h, d->H);
    if ((uintptr_t)params & 255) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "params must be 256-byte aligned");
    return DRNMF_OK;
}

// A wavefront of T + K - 1 diagonals (the forwards count up, the BPTT counts DOWN: its kernel writes d - 1), two
// per graph frame: the first launch reads counter 0 and sets counter 1, the second the other way round (nobody
// reads a counter in the launch that writes it).  An odd diagonal count ends on one launch whose workgroups all
// exit at once.  Args: LstmStepArgs or LstmBwdArgs.
template <class Args>
static int32_t lstm_wavefront(drnmf_handle_t h, hipStream_t stream, GraphKind kind,
                              const std::vector<uint64_t>& key, int T, int K, const void* kernel, dim3 grid,
                              const Args& base, int* ctr) {
    auto frame = [&](Launcher& chain, int) -> int32_t {
        for (int p = 0; p < 2; ++p) {
            Args a = base;
            a.d_rd = ctr + 16 * p;
            a.d_wr = ctr + 16 * (1 - p);
            void* kp[1] = {&a};
            DRNMF_HIP(h, chain.add(kernel, grid, dim3(64 * LSTM_NW), kp));
        }
        return DRNMF_OK;
    };
    const int diagonals = T + K - 1, frames = (diagonals + 1) / 2;
    const int fpg = frames < 64 ? frames : 64;
    return replay_frames(h, stream, kind, key, {fpg, 1}, 0, frames, frame);
}

namespace {     // (defined with the training kernels below)
__global__ void lstm_stash_init_kernel(float* __restrict__ zst, float* __restrict__ cst, float* __restrict__ hst,
                                       int Bp, int T, size_t zk, size_t RS, int NC, int Hc, int Hq);
}

// One forward's buffers, carved by the entry from its own layout (LstmLayout or LstmTrainLayout)
struct LstmFwdViews {
    float* xz;
    unsigned char* valid;
    float* xproj;
    float* hring;
    float* cring;
    f16* h16;                  // operand_f16 only, else NULL
    int* ctr;
    size_t rows;               // of xz / valid / xproj: B T, or B (T + 1) in the training layout
    float* zst;                // the training stash (lstm_step_kernel<true>), or all NULL / 0
    float* cst;
    float* hst;
    size_t zk, RS;
};

// Everything of a forward behind its pack launch: entering state, (training) the stash's zero rows and entering
// state, input projection, the wavefront and the state behind it.  st == nullptr: zero state in, none out; else a
// *_stateful entry.  The state kernels run on the stream before and behind the replayed frames, never inside
// them: the graphs hold no state pointer (the cache key has none), and both entry points of a kind replay the
// same graphs.  The entering state of a training call also goes into row b (T + 1) of the stash, where the BPTT
// finds it: a constant of the gradient.
static int32_t lstm_forward_run(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const LstmLayout& L,
                                const LstmFwdViews& V, const void* params, float* h_out, int32_t ld_h,
                                void* workspace, hipStream_t stream, const LstmState* st, const void* step,
                                GraphKind kind) {
    const char* pb = (const char*)params;
    const size_t nring = (size_t)d->K * 2 * L.Bp * L.Hc;
    if (st)
        hipLaunchKernelGGL(lstm_state_scatter_kernel, dim3((unsigned)((nring + 255) / 256)), dim3(256), 0, stream,
                           V.hring, V.cring, V.h16, V.ctr, st->initial_h, st->initial_c, nring, d->B, d->H, L.Bp,
                           L.Hc);
    else
        hipLaunchKernelGGL(lstm_init_kernel, dim3((unsigned)((nring + 255) / 256)), dim3(256), 0, stream, V.hring,
                           V.cring, V.h16, V.ctr, nring);
    if (V.zst) {
        hipLaunchKernelGGL(lstm_stash_init_kernel, dim3((unsigned)(L.Bp + 1), (unsigned)d->K), dim3(256), 0, stream,
                           V.zst, V.cst, V.hst, L.Bp, d->T, V.zk, V.RS, L.NC, L.Hc, L.Hq);
        if (st && (st->initial_h || st->initial_c)) {
            const size_t ns = (size_t)d->K * d->B * d->H;
            hipLaunchKernelGGL(lstm_stash_state_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, stream,
                               V.cst, V.hst, st->initial_h, st->initial_c, ns, d->B, d->H, d->T, V.RS, L.Hc, L.Hq);
        }
    }
    DRNMF_HIP(h, hipGetLastError());
    {
        gemm::Operands g;
        g.A = V.xz;
        g.Bt = (const float*)(pb + L.off_k0t);
        g.M = (int64_t)V.rows;
        g.N = L.NC;
        g.K = L.Fq;
        g.lda = g.ldb = L.Fq;
        DRNMF_HIP(h, gemm::launch(g, EpiLstmXproj{V.xproj, (const float*)(pb + L.off_bias), L.NC}, stream));
    }

    LstmStepArgs base{};
    base.M = (const float*)pb;
    base.bias = (const float*)(pb + L.off_bias);
    base.xproj = V.xproj;
    base.valid = V.valid;
    base.hring = V.hring;
    base.cring = V.cring;
    base.out = h_out;
    base.B = d->B; base.T = d->T; base.H = d->H; base.K = d->K;
    base.Bp = L.Bp; base.Hc = L.Hc; base.numU = L.numU; base.NC = L.NC;
    base.act = d->recurrent_activation;
    base.ld_h = ld_h;
    base.zst = V.zst; base.cst = V.cst; base.hst = V.hst; base.zk = V.zk; base.Hq = L.Hq;
    base.h16 = V.h16;
    const dim3 grid((unsigned)L.numU, (unsigned)(L.Bp / 16), (unsigned)d->K);
    std::vector<uint64_t> key = {
        (uint64_t)d->B, (uint64_t)d->T, (uint64_t)d->F, (uint64_t)d->H, (uint64_t)d->K,
        (uint64_t)d->recurrent_activation, (uint64_t)(uintptr_t)params, (uint64_t)(uintptr_t)h_out, (uint64_t)ld_h,
        (uint64_t)(uintptr_t)workspace};
    if (kind == GraphKind::Lstm) key.push_back((uint64_t)d->operand_f16);    // (LstmTrain refuses operand_f16)
    int32_t rc = lstm_wavefront(h, stream, kind, key, d->T, d->K, step, grid, base, V.ctr);
    if (rc) return rc;
    return lstm_store_state(h, d, L, V.hring, V.cring, st, stream);
}

static int32_t lstm_forward_impl(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* x, float mask_value,
                                 const void* params, float* h_out, int32_t ld_h, void* workspace,
                                 size_t workspace_bytes, void* stream_, const LstmState* st, const char* what) {
    if (!h) return DRNMF_ERR_INVALID_ARG;
    int rc = validate_lstm_desc(h, d, true);
    if (rc) return rc;
    ++h->call_seq;                   // (a top-level call: the graphs it takes are pinned until it returns)
    if (!x || !params || !h_out || !workspace)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: NULL pointer argument", what);
    if (ld_h < d->H) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: ld_h %d < H %d", what, ld_h, d->H);
    const LstmLayout L = lstm_layout(d);
    if (workspace_bytes < L.ws_total)
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "%s: workspace %zu < required %zu", what, workspace_bytes,
                   L.ws_total);
    if (((uintptr_t)workspace & 255) || ((uintptr_t)params & 255))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "workspace/params must be 256-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    LstmFwdViews V{};
    V.xz = (float*)(ws + L.off_xz);
    V.valid = (unsigned char*)(ws + L.off_valid);
    V.xproj = (float*)(ws + L.off_xproj);
    V.hring = (float*)(ws + L.off_h);
    V.cring = (float*)(ws + L.off_c);
    V.h16 = L.half ? (f16*)(ws + L.off_h16) : nullptr;
    V.ctr = (int*)(ws + L.off_ctr);
    V.rows = (size_t)d->B * d->T;
    hipLaunchKernelGGL(lstm_pack_x_kernel, dim3((unsigned)((V.rows + 3) / 4)), dim3(256), 0, stream, x, V.xz,
                       V.valid, mask_value, V.rows, d->F, L.Fq);
    const void* step = L.half ? (const void*)&lstm_step_kernel<false, true>
                              : (const void*)&lstm_step_kernel<false, false>;
    return lstm_forward_run(h, d, L, V, params, h_out, ld_h, workspace, stream, st, step, GraphKind::Lstm);
}

extern "C" int32_t drnmf_lstm_forward(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* x,
                                      float mask_value, const void* params, float* h_out, int32_t ld_h,
                                      void* workspace,
                                      size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    return lstm_forward_impl(h, d, x, mask_value, params, h_out, ld_h, workspace, workspace_bytes, stream_,
                             nullptr, "lstm_forward");
}

extern "C" int32_t drnmf_lstm_forward_stateful(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* x,
                                               float mask_value, const void* params, const float* initial_h,
                                               const float* initial_c, float* final_h, float* final_c,
                                               float* h_out, int32_t ld_h, void* workspace,
                                               size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    const LstmState st{initial_h, initial_c, final_h, final_c};
    return lstm_forward_impl(h, d, x, mask_value, params, h_out, ld_h, workspace, workspace_bytes, stream_, &st,
                             "lstm_forward_stateful");
}

// Columns of a hidden row that the head's products contract.  With ld_h >= round_up(H, 4) they take the padding
// columns too (against zero rows of W_out^T): K and lda are then multiples of 4 and the gemm takes its vectorised
// path (and the split-operand one in bf16x3 mode).
static int lstm_head_k(const drnmf_lstm_desc_t* d, const LstmLayout& L, int32_t ld_h) {
    return ld_h >= L.Hq ? L.Hq : d->H;
}

// out [B T][F] = sigmoid(hidden . W_out + b_out)
static hipError_t lstm_head_product(const drnmf_lstm_desc_t* d, const LstmLayout& L, const float* hidden,
                                    int32_t ld_h, const void* params, float* out, hipStream_t stream) {
    const char* pb = (const char*)params;
    gemm::Operands g;
    g.A = hidden;
    g.Bt = (const float*)(pb + L.off_wo);
    g.M = (int64_t)d->B * d->T;
    g.N = d->F;
    g.K = lstm_head_k(d, L, ld_h);
    g.lda = ld_h;
    g.ldb = L.Hq;
    return gemm::launch(g, EpiLstmHead{out, (const float*)(pb + L.off_bo), d->F}, stream);
}

extern "C" int32_t drnmf_lstm_head_forward(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* hidden,
                                           int32_t ld_h, const void* params, float* out, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    int rc = validate_lstm_desc(h, d, true);
    if (rc) return rc;
    if (!hidden || !params || !out) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "lstm_head_forward: NULL pointer argument");
    rc = lstm_check_ld_params(h, d, ld_h, params, "lstm_head_forward");
    if (rc) return rc;
    DRNMF_HIP(h, lstm_head_product(d, lstm_layout(d), hidden, ld_h, params, out, (hipStream_t)stream_));
    return DRNMF_OK;
}

// ---- training: forward with stash, loss head + its backward, BPTT as a reverse wavefront -------------------
//
// The three training entry points share one workspace (drnmf_lstm_train_workspace_bytes), run in this order on
// it: drnmf_lstm_train_forward -> drnmf_lstm_loss_head_backward -> drnmf_lstm_backward.
//
// Training layout of the frames: row b (T + 1) + t + 1 holds frame t of sequence b, row b (T + 1) is a zero
// frame.  The masked input xz, xproj, valid and the stash (z, c, h of every layer) use it, so that the
// recurrent-kernel gradient sum_t h_{k,t-1}^T dz_{k,t} is ONE gemm_tn over B (T + 1) rows with the dz operand
// one row ahead (a masked frame copies h, so row t is the state that entered step t).  The stash blocks have
// Bp (T + 1) rows per layer (the BPTT's 16-row tiles read padded rows), the z / dz block one more zero row.
//
// BPTT [K2.0.4-memory: Theano's autodiff of the masked K.rnn]: (k, t) needs (k + 1, t) and (k, t + 1) only,
// so one launch per diagonal d = k + t, from T + K - 2 down to 0.  Workgroup (tile of 32 units, 16 rows, k)
// contracts [dz_{k+1,t} | dz_{k,t+1}] (top layer: dz_{K-1,t+1} alone) with the transposed stacked matrix
// [kernel_{k+1}; recurrent_k]^T and adds, in its epilogue, d_hidden_t (top layer) and the pass-through carried
// from a masked (k, t + 1).  With G_h that sum and G_c the carried dc:
//   valid (k, t):  dc = G_c + G_h o (1 - tanh^2 c_t);  dz_i = dc tanh(z_c) s'(z_i), dz_f = dc c_{t-1} s'(z_f),
//                  dz_c = dc i (1 - tanh^2 z_c), dz_o = G_h tanh(c_t) s'(z_o);  carried to t - 1: dh 0, dc f;
//   masked (k, t): dz = 0;  carried to t - 1: dh = G_h, dc = G_c (both states were copies).
// s' of hard_sigmoid is 0.2 on the CLOSED interval 0 <= 0.2 z + 0.5 <= 1 (Theano's clip), hence z is stashed,
// not the gate.  dz overwrites z in place: only (k, t) reads z_{k,t}, and dz_{k,t} is read one diagonal later.
namespace {

constexpr int LSTM_WG_SPLITS = 32;     // upper bound of the split-K count of a weight-gradient product

struct LstmTrainLayout {
    LstmLayout L;
    int NB, NBc;                       // BPTT output tiles of 32 units, NB * 32
    size_t R1, RS, zk, part_floats, cpart_floats;
    size_t off_xz, off_valid, off_xproj, off_h, off_c, off_ctr, off_z, off_cst, off_hst;
    size_t off_s, off_dpre, off_wop, off_lpart, off_mt, off_ph, off_pc, off_bctr, off_part, off_cpart, total;
};

LstmTrainLayout lstm_train_layout(const drnmf_lstm_desc_t* d) {
    LstmTrainLayout W;
    W.L = lstm_layout(d);
    const LstmLayout& L = W.L;
    const size_t B = d->B > 0 ? d->B : 0, T = d->T > 0 ? d->T : 0, K = d->K, F = d->F, H = d->H;
    W.NB = (d->H + 31) / 32;
    W.NBc = W.NB * 32;
    W.R1 = B * (T + 1);
    W.RS = (size_t)L.Bp * (T + 1);
    W.zk = W.RS + 1;
    const size_t mmax = (size_t)(L.Fq > L.Hq ? L.Fq : L.Hq), nmax = (size_t)(L.NC > L.Fq ? L.NC : L.Fq);
    W.part_floats = (size_t)LSTM_WG_SPLITS * mmax * nmax;
    W.cpart_floats = (size_t)LSTM_WG_SPLITS * nmax;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += round_up_sz(bytes, 256); return at; };
    W.off_xz = take(W.R1 * L.Fq * 4);
    W.off_valid = take(W.R1);
    W.off_xproj = take(W.R1 * L.NC * 4);
    W.off_h = take(K * 2 * L.Bp * L.Hc * 4);
    W.off_c = take(K * 2 * L.Bp * L.Hc * 4);
    W.off_ctr = take(256);
    W.off_z = take(K * W.zk * L.NC * 4);
    W.off_cst = take(K * W.RS * L.Hc * 4);
    W.off_hst = take(K * W.RS * L.Hq * 4);
    W.off_s = take(B * T * F * 4);
    W.off_dpre = take(B * T * L.Fq * 4);
    W.off_wop = take(H * L.Fq * 4);
    W.off_lpart = take((B * T + 3) / 4 * 2 * 4);
    W.off_mt = take(K * 2 * L.NC * W.NBc * 4);
    W.off_ph = take(K * 2 * L.Bp * W.NBc * 4);
    W.off_pc = take(K * 2 * L.Bp * W.NBc * 4);
    W.off_bctr = take(256);
    W.off_part = take(W.part_floats * 4);
    W.off_cpart = take(W.cpart_floats * 4);
    W.total = o;
    return W;
}

// x [B][T][F] -> xz [B (T+1)][Fq] and valid in the training layout (zero frame at row b (T + 1), not valid)
__global__ void __launch_bounds__(256)
lstm_pack_x_train_kernel(const float* __restrict__ x, float* __restrict__ xz, unsigned char* __restrict__ valid,
                         float mask_value, size_t rows, int T, int F, int Fq) {
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + wv;
    if (row >= rows) return;
    const size_t b = row / (T + 1), j = row % (T + 1);
    float* dst = xz + row * Fq;
    if (j == 0) {
        for (int f = l; f < Fq; f += 64) dst[f] = 0.f;
        if (l == 0) valid[row] = 0;
        return;
    }
    const float* src = x + (b * T + j - 1) * F;
    bool any = false;
    for (int f = l; f < F; f += 64) any |= (src[f] != mask_value);
    any = __any(any);
    for (int f = l; f < Fq; f += 64) dst[f] = (any && f < F) ? src[f] : 0.f;
    if (l == 0) valid[row] = any ? 1 : 0;
}

// zero rows of the stash: per layer, row b (T + 1) of z / c / h for every b < Bp and z's trailing row
__global__ void __launch_bounds__(256)
lstm_stash_init_kernel(float* __restrict__ zst, float* __restrict__ cst, float* __restrict__ hst, int Bp, int T,
                       size_t zk, size_t RS, int NC, int Hc, int Hq) {
    const int k = blockIdx.y, b = blockIdx.x;      // b == Bp: the trailing z row
    const size_t T1 = (size_t)T + 1;
    float* zr = zst + ((size_t)k * zk + (size_t)b * T1) * NC;
    for (int i = threadIdx.x; i < NC; i += 256) zr[i] = 0.f;
    if (b == Bp) return;
    const size_t srow = (size_t)k * RS + (size_t)b * T1;
    for (int i = threadIdx.x; i < Hc; i += 256) cst[srow * Hc + i] = 0.f;
    for (int i = threadIdx.x; i < Hq; i += 256) hst[srow * Hq + i] = 0.f;
}

// ---- loss head --------------------------------------------------------------------------------------------

// w_out [H][F] -> [H][Fq] (zero columns F .. Fq-1): the "Bt" of d_hidden = dpre . w_out^T on the vector path
__global__ void __launch_bounds__(256)
lstm_pad_wo_kernel(const float* __restrict__ wo, float* __restrict__ out, int F, int Fq, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t r = i / Fq;
    const int f = (int)(i % Fq);
    out[i] = f < F ? wo[r * F + f] : 0.f;
}

// mse_of_masked (enhance.py:1260-1312): one wave per frame r = b T + t, xm = the Masking layer's output (the
// training-layout xz row), s = sigmoid output, e = xm s - y:  loss_r = w mean_F e^2,
// dpre = w (2 / F) e xm s (1 - s) (zeros in the padding bins).  Block partials {sum loss_r, #(w != 0)}.
__global__ void __launch_bounds__(256)
lstm_loss_rows_kernel(const float* __restrict__ xz, const float* __restrict__ S, const float* __restrict__ y,
                      const float* __restrict__ w, float* __restrict__ dpre, float* __restrict__ part,
                      size_t rows, int T, int F, int Fq) {
    __shared__ float sl[4], sc[4];
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + wv;
    float acc = 0.f, cnt = 0.f;
    if (row < rows) {
        const size_t b = row / T, t = row % T;
        const float* xm = xz + (b * (T + 1) + t + 1) * Fq;
        const float* s = S + row * F;
        const float* yy = y + row * F;
        const float wr = w[row], g = wr * (2.f / (float)F);
        float* dp = dpre + row * Fq;
        for (int f = l; f < Fq; f += 64) {
            float v = 0.f;
            if (f < F) {
                const float xs = xm[f] * s[f], e = xs - yy[f];
                acc += e * e;
                v = g * e * xs * (1.f - s[f]);
            }
            dp[f] = v;
        }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        acc = wr * (acc / (float)F);
        cnt = wr != 0.f ? 1.f : 0.f;
    }
    if (l == 0) { sl[wv] = acc; sc[wv] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = (sl[0] + sl[1]) + (sl[2] + sl[3]);
        part[2 * (size_t)blockIdx.x + 1] = (sc[0] + sc[1]) + (sc[2] + sc[3]);
    }
}

// lstm_loss_rows_kernel's dpre for a GIVEN cotangent of the head's output (drnmf_lstm_head_backward_cot):
// dpre = d_mask s (1 - s), zeros in the padding bins; one wave per frame
__global__ void __launch_bounds__(256)
lstm_cot_rows_kernel(const float* __restrict__ d_mask, int64_t ld_dm, const float* __restrict__ S,
                     float* __restrict__ dpre, size_t rows, int F, int Fq) {
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + wv;
    if (row >= rows) return;
    const float* dm = d_mask + row * (size_t)ld_dm;
    const float* s = S + row * F;
    float* dp = dpre + row * Fq;
    for (int f = l; f < Fq; f += 64) dp[f] = f < F ? dm[f] * s[f] * (1.f - s[f]) : 0.f;
}

// fixed-order fp64 sum of the block partials (deterministic)
__global__ void __launch_bounds__(256)
lstm_loss_final_kernel(const float* __restrict__ part, int64_t nblocks, float* __restrict__ sums) {
    __shared__ double s0[256], s1[256];
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < nblocks; i += 256) {
        a += (double)part[2 * i];
        b += (double)part[2 * i + 1];
    }
    s0[threadIdx.x] = a;
    s1[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s0[threadIdx.x] += s0[threadIdx.x + o];
            s1[threadIdx.x] += s1[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { sums[0] = (float)s0[0]; sums[1] = (float)s1[0]; }
}

struct EpiLstmDh {      // d_hidden = dpre . w_out^T
    float* out;
    int ld;
    __device__ f32x2 pre(int64_t, int) const { return f32x2{0.f, 0.f}; }
    __device__ void operator()(int64_t row, int col, float acc, f32x2) const { out[row * ld + col] = acc; }
};

// ---- weight gradients -------------------------------------------------------------------------------------

struct EpiLstmPart {    // split-K partial tiles of gemm_tn, summed by lstm_sum_parts_kernel in a fixed order
    float* P;
    int ld;
    size_t stride;
    __device__ float pre(int, int, int) const { return 0.f; }
    __device__ void operator()(int split, int m, int n, float acc, float) const {
        P[split * stride + (size_t)m * ld + n] = acc;
    }
};

// column sums over rows, per split (fixed order)
__global__ void __launch_bounds__(256)
lstm_colsum_kernel(const float* __restrict__ A, float* __restrict__ part, int64_t rows, int N, int64_t ld) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int sp = blockIdx.y, nsp = gridDim.y;
    if (n >= N) return;
    const int64_t per = (rows + nsp - 1) / nsp;
    int64_t r1 = (sp + 1) * per;
    if (r1 > rows) r1 = rows;
    float s = 0.f;
    for (int64_t r = sp * per; r < r1; ++r) s += A[r * ld + n];
    part[(size_t)sp * N + n] = s;
}

// out [Mr][Nr] = sum over the splits (in order) of P[s][m][col]; H > 0: Nr = 4H Keras gate columns, col = the
// packed column of (gate g, unit u) = (u / 8) 32 + 8 g + u % 8; H == 0: col = the output column itself
__global__ void __launch_bounds__(256)
lstm_sum_parts_kernel(const float* __restrict__ P, float* __restrict__ out, int Mr, int Nr, int ldp,
                      size_t pstride, int splits, int H) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)Mr * Nr) return;
    const int m = (int)(i / Nr), c = (int)(i % Nr);
    int col = c;
    if (H > 0) {
        const int g = c / H, u = c % H;
        col = (u >> 3) * 32 + g * 8 + (u & 7);
    }
    const float* p = P + (size_t)m * ldp + col;
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += p[(size_t)k * pstride];
    out[i] = s;
}

// ---- BPTT -------------------------------------------------------------------------------------------------

// Transposed stacked matrix of layer k in the operand order of lstm_bwd_step_kernel (the packing of
// lstm_pack_step_kernel with 32-unit output tiles): contraction rows = packed gate columns of
// kernel_{k+1} (k < K-1) then of recurrent_k; output column n = unit n of layer k.
__global__ void __launch_bounds__(256)
lstm_pack_bwd_kernel(const float* __restrict__ kern_next, const float* __restrict__ rec, float* __restrict__ Mt,
                     int H, int NC, int NB, int rows) {
    const int NBc = NB * 32;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)rows * NBc) return;
    const int i = (int)(idx / NBc), n = (int)(idx % NBc);
    const bool two = kern_next != nullptr;
    const float* src = two && i < NC ? kern_next : rec;
    const int p = two && i >= NC ? i - NC : i;
    const int g = (p & 31) >> 3, u = (p >> 5) * LSTM_UNITS + (p & 7);
    const float v = (u < H && n < H) ? src[(size_t)n * 4 * H + (size_t)g * H + u] : 0.f;
    const int c = i >> 4, kk = i & 15, q = kk >> 2, s = kk & 3;
    const int ab = n >> 5, pc = n & 31;
    Mt[((size_t)c * NB + ab) * 512 + (pc >> 4) * 256 + (q * 16 + (pc & 15)) * 4 + s] = v;
}

__global__ void __launch_bounds__(256)
lstm_bwd_init_kernel(float* __restrict__ ph, float* __restrict__ pc, int* ctr, size_t n, int d0) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) { ctr[0] = d0; ctr[16] = d0; }
    if (i < n) { ph[i] = 0.f; pc[i] = 0.f; }
}

__device__ __forceinline__ float gate_grad(float v, int act) {    // d gate_act / dv
    if (act == DRNMF_ACT_SIGMOID) {
        const float s = 1.f / (1.f + expf(-v));
        return s * (1.f - s);
    }
    const float p = 0.2f * v + 0.5f;
    return (p >= 0.f && p <= 1.f) ? 0.2f : 0.f;
}

struct LstmBwdArgs {
    const float* Mt;           // [K][2 NC rows][NBc] packed (lstm_pack_bwd_kernel)
    float* Z;                  // [K][zk][NC]: z in, dz out (training layout)
    const float* cst;          // [K][Bp (T+1)][Hc]
    const unsigned char* valid;   // [B (T+1)]
    const float* dh;           // [B][T][H]: d loss / d (last layer's output)
    float* ph;                 // [K][2][Bp][NBc]: dh carried past a masked frame, slot t & 1 written by (k, t)
    float* pc;                 // [K][2][Bp][NBc]: dc carried to t - 1
    const int* d_rd;
    int* d_wr;
    size_t zk;
    int B, T, H, K, Bp, Hc, NB, NC, act;
};

// One launch = one diagonal d (descending): workgroup (ab, mb, k) computes (k, t = d - k) for rows
// 16 mb .. 16 mb + 15 and units 32 ab .. 32 ab + 31.  Contraction as lstm_step_kernel (exact-fp32 MFMA, split
// over the waves, reduced through LDS in a fixed order); the A rows are dz rows of the stash.
__global__ void __launch_bounds__(64 * LSTM_NW) lstm_bwd_step_kernel(const LstmBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float red[LSTM_NW * 16 * 32];
    const int ab = blockIdx.x, mb = blockIdx.y, k = blockIdx.z;
    const int d = *a.d_rd;
    if (ab == 0 && mb == 0 && k == 0 && threadIdx.x == 0) *a.d_wr = d - 1;
    const int t = d - k;
    if (t < 0 || t >= a.T) return;
    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63, j = l & 15, q = l >> 4;
    const bool top = k == a.K - 1;
    const int nq = a.NC / 16, nch = top ? nq : 2 * nq;
    const size_t T1 = (size_t)a.T + 1;
    const size_t seq = (size_t)(mb * 16 + j) * T1;
    const float* next = a.Z + ((size_t)k * a.zk + seq + t + 2) * a.NC + 4 * q;                 // dz_{k,t+1}
    const float* above = top ? next : a.Z + ((size_t)(k + 1) * a.zk + seq + t + 1) * a.NC + 4 * q;  // dz_{k+1,t}
    const float* brow = a.Mt + (size_t)k * 2 * a.NC * (a.NB * 32) + (size_t)ab * 512 + l * 4;
    const size_t bstep = (size_t)a.NB * 512;

    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = w; c0 < nch; c0 += LSTM_NW * LSTM_G) {
        f32x4 av[LSTM_G], b0[LSTM_G], b1[LSTM_G];
#pragma unroll
        for (int g = 0; g < LSTM_G; ++g) {
            const int c = c0 + LSTM_NW * g;
            const int cc = c < nch ? c : nch - 1;
            const float* ap = top ? next + 16 * cc : (cc < nq ? above + 16 * cc : next + 16 * (cc - nq));
            av[g] = *(const f32x4*)ap;
            b0[g] = *(const f32x4*)(brow + (size_t)cc * bstep);
            b1[g] = *(const f32x4*)(brow + (size_t)cc * bstep + 256);
            if (c >= nch) av[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int g = 0; g < LSTM_G; ++g)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                acc0 = mfma16(av[g][s], b0[g][s], acc0);
                acc1 = mfma16(av[g][s], b1[g][s], acc1);
            }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        red[(w * 16 + 4 * q + v) * 32 + j] = acc0[v];
        red[(w * 16 + 4 * q + v) * 32 + 16 + j] = acc1[v];
    }
    __syncthreads();

    // cell backward: thread = row r, units uu and uu + 16 of the tile
    const int r = tid >> 4, b = mb * 16 + r;
    const int NBc = a.NB * 32;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int uu = (tid & 15) + 16 * half, n = ab * 32 + uu;
        float gh = 0.f;
#pragma unroll
        for (int ww = 0; ww < LSTM_NW; ++ww) gh += red[(ww * 16 + r) * 32 + uu];
        const size_t e_next = (((size_t)k * 2 + ((t + 1) & 1)) * a.Bp + b) * NBc + n;
        const size_t e_cur = (((size_t)k * 2 + (t & 1)) * a.Bp + b) * NBc + n;
        gh += a.ph[e_next];
        const float gc = a.pc[e_next];
        const bool keep = b < a.B && n < a.H;
        if (top && keep) gh += a.dh[((size_t)b * a.T + t) * a.H + n];
        const size_t zrow = (size_t)k * a.zk + (size_t)b * T1 + t + 1;
        float* zp = a.Z + zrow * a.NC + (n >> 3) * 32 + (n & 7);
        if (keep && a.valid[(size_t)b * T1 + t + 1]) {
            const float z0 = zp[0], z1 = zp[8], z2 = zp[16], z3 = zp[24];
            const size_t srow = (size_t)k * a.Bp * T1 + (size_t)b * T1 + t + 1;
            const float c = a.cst[srow * a.Hc + n], cp = a.cst[(srow - 1) * a.Hc + n];
            const float ig = gate_act(z0, a.act), fg = gate_act(z1, a.act), og = gate_act(z3, a.act);
            const float gt = tanhf(z2), tc = tanhf(c);
            const float dc = gc + gh * og * (1.f - tc * tc);
            zp[0] = dc * gt * gate_grad(z0, a.act);
            zp[8] = dc * cp * gate_grad(z1, a.act);
            zp[16] = dc * ig * (1.f - gt * gt);
            zp[24] = gh * tc * gate_grad(z3, a.act);
            a.ph[e_cur] = 0.f;
            a.pc[e_cur] = dc * fg;
        } else {
            if (n < a.NC / 4) { zp[0] = 0.f; zp[8] = 0.f; zp[16] = 0.f; zp[24] = 0.f; }
            a.ph[e_cur] = keep ? gh : 0.f;
            a.pc[e_cur] = keep ? gc : 0.f;
        }
    }
}

int validate_train_call(drnmf_handle_t h, const drnmf_lstm_desc_t* d, void* workspace, size_t workspace_bytes,
                        const char* what, LstmTrainLayout* W) {
    int rc = validate_lstm_desc(h, d, true);
    if (rc) return rc;
    if (d->operand_f16)
        DRNMF_FAIL(h, DRNMF_ERR_UNSUPPORTED,
                   "%s: operand_f16 = 1 is inference only (train with operand_f16 = 0)", what);
    *W = lstm_train_layout(d);
    if (!workspace) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: NULL workspace", what);
    if (workspace_bytes < W->total)
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "%s: workspace %zu < required %zu", what, workspace_bytes, W->total);
    if ((uintptr_t)workspace & 255) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "workspace must be 256-byte aligned");
    return DRNMF_OK;
}

// C[M x N] = A^T B over `rows` rows (split-K partials in the workspace) -> out [Mr][Nr] (Keras gate order when
// H > 0, see lstm_sum_parts_kernel)
hipError_t lstm_tn_product(const LstmTrainLayout& W, char* ws, const float* A, int64_t lda, int M, const float* Bm,
                           int64_t ldb, int N, int64_t rows, float* out, int Mr, int Nr, int H, hipStream_t stream) {
    float* part = (float*)(ws + W.off_part);
    int splits = gemm_tn::pick_splits(M, N, rows, LSTM_WG_SPLITS);
    gemm_tn::Operands g{A, Bm, rows, M, N, lda, ldb};
    hipError_t e = gemm_tn::launch(g, EpiLstmPart{part, N, (size_t)M * N}, splits, stream);
    if (e != hipSuccess) return e;
    const size_t n = (size_t)Mr * Nr;
    hipLaunchKernelGGL(lstm_sum_parts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, part, out,
                       Mr, Nr, N, (size_t)M * N, splits, H);
    return hipGetLastError();
}

hipError_t lstm_colsum(const LstmTrainLayout& W, char* ws, const float* A, int64_t ld, int N, int64_t rows,
                       float* out, int Nr, int H, hipStream_t stream) {
    float* part = (float*)(ws + W.off_cpart);
    int splits = LSTM_WG_SPLITS;
    while (splits > 1 && rows / splits < 64) splits >>= 1;
    hipLaunchKernelGGL(lstm_colsum_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)splits), dim3(256), 0,
                       stream, A, part, rows, N, ld);
    hipLaunchKernelGGL(lstm_sum_parts_kernel, dim3((unsigned)((Nr + 255) / 256)), dim3(256), 0, stream, part, out,
                       1, Nr, N, (size_t)N, splits, H);
    return hipGetLastError();
}

}  // namespace

extern "C" size_t drnmf_lstm_train_workspace_bytes(const drnmf_lstm_desc_t* d) {
    if (!d || d->B <= 0 || d->T <= 0 || d->F <= 0 || d->H <= 0 || d->K <= 0) return 0;
    if (d->operand_f16) return 0;          // inference only: every training entry point refuses the descriptor
    return lstm_train_layout(d).total;
}

static int32_t lstm_train_forward_impl(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* x,
                                       float mask_value, const void* params, float* h_out, int32_t ld_h,
                                       void* workspace, size_t workspace_bytes, void* stream_,
                                       const LstmState* st, const char* what) {
    if (!h) return DRNMF_ERR_INVALID_ARG;
    LstmTrainLayout W;
    int rc = validate_train_call(h, d, workspace, workspace_bytes, what, &W);
    if (rc) return rc;
    ++h->call_seq;
    if (!x || !params || !h_out) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: NULL pointer argument", what);
    rc = lstm_check_ld_params(h, d, ld_h, params, what);
    if (rc) return rc;
    const LstmLayout& L = W.L;
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    LstmFwdViews V{};
    V.xz = (float*)(ws + W.off_xz);
    V.valid = (unsigned char*)(ws + W.off_valid);
    V.xproj = (float*)(ws + W.off_xproj);
    V.hring = (float*)(ws + W.off_h);
    V.cring = (float*)(ws + W.off_c);
    V.ctr = (int*)(ws + W.off_ctr);
    V.rows = W.R1;
    V.zst = (float*)(ws + W.off_z);
    V.cst = (float*)(ws + W.off_cst);
    V.hst = (float*)(ws + W.off_hst);
    V.zk = W.zk;
    V.RS = W.RS;
    hipLaunchKernelGGL(lstm_pack_x_train_kernel, dim3((unsigned)((W.R1 + 3) / 4)), dim3(256), 0, stream, x, V.xz,
                       V.valid, mask_value, W.R1, d->T, d->F, L.Fq);
    return lstm_forward_run(h, d, L, V, params, h_out, ld_h, workspace, stream, st,
                            (const void*)&lstm_step_kernel<true, false>, GraphKind::LstmTrain);
}

extern "C" int32_t drnmf_lstm_train_forward(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* x,
                                            float mask_value, const void* params, float* h_out, int32_t ld_h,
                                            void* workspace, size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    return lstm_train_forward_impl(h, d, x, mask_value, params, h_out, ld_h, workspace, workspace_bytes, stream_,
                                   nullptr, "lstm_train_forward");
}

extern "C" int32_t drnmf_lstm_train_forward_stateful(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* x,
                                                     float mask_value, const void* params,
                                                     const float* initial_h, const float* initial_c,
                                                     float* final_h, float* final_c, float* h_out, int32_t ld_h,
                                                     void* workspace, size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    const LstmState st{initial_h, initial_c, final_h, final_c};
    return lstm_train_forward_impl(h, d, x, mask_value, params, h_out, ld_h, workspace, workspace_bytes, stream_,
                                   &st, "lstm_train_forward_stateful");
}

// The three products behind dpre (W.off_dpre, [B T][Fq] with zero padding bins), shared by the fused loss head and
// drnmf_lstm_head_backward_cot: d_hidden = dpre . w_out^T, d_w_out = hidden^T dpre, d_b_out = column sums of dpre
static int32_t lstm_head_products(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const LstmTrainLayout& W, char* ws,
                                  const float* hidden, int32_t ld_h, const float* w_out, float* d_hidden,
                                  float* d_w_out, float* d_b_out, hipStream_t stream) {
    const LstmLayout& L = W.L;
    const int64_t rows = (int64_t)d->B * d->T;
    float* dpre = (float*)(ws + W.off_dpre);
    float* wop = (float*)(ws + W.off_wop);
    const size_t nw = (size_t)d->H * L.Fq;
    hipLaunchKernelGGL(lstm_pad_wo_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, stream, w_out, wop,
                       d->F, L.Fq, nw);
    DRNMF_HIP(h, hipGetLastError());
    {   // d_hidden [B T][H] = dpre . w_out^T
        gemm::Operands g;
        g.A = dpre;
        g.Bt = wop;
        g.M = rows;
        g.N = d->H;
        g.K = L.Fq;
        g.lda = g.ldb = L.Fq;
        DRNMF_HIP(h, gemm::launch(g, EpiLstmDh{d_hidden, d->H}, stream));
    }
    DRNMF_HIP(h, lstm_tn_product(W, ws, hidden, ld_h, lstm_head_k(d, L, ld_h), dpre, L.Fq, L.Fq, rows, d_w_out,
                                 d->H, d->F, 0, stream));
    DRNMF_HIP(h, lstm_colsum(W, ws, dpre, L.Fq, L.Fq, rows, d_b_out, d->F, 0, stream));
    return DRNMF_OK;
}

extern "C" int32_t drnmf_lstm_loss_head_backward(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* y,
                                                 const float* w, const float* hidden, int32_t ld_h,
                                                 const void* params, const float* w_out, float* sums,
                                                 float* d_hidden, float* d_w_out, float* d_b_out, void* workspace,
                                                 size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    LstmTrainLayout W;
    int rc = validate_train_call(h, d, workspace, workspace_bytes, "lstm_loss_head_backward", &W);
    if (rc) return rc;
    if (!y || !w || !hidden || !params || !w_out || !sums || !d_hidden || !d_w_out || !d_b_out)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "lstm_loss_head_backward: NULL pointer argument");
    rc = lstm_check_ld_params(h, d, ld_h, params, "lstm_loss_head_backward");
    if (rc) return rc;
    const LstmLayout& L = W.L;
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    const int64_t rows = (int64_t)d->B * d->T;
    float* S = (float*)(ws + W.off_s);
    float* dpre = (float*)(ws + W.off_dpre);
    float* lpart = (float*)(ws + W.off_lpart);
    DRNMF_HIP(h, lstm_head_product(d, L, hidden, ld_h, params, S, stream));
    const int64_t nblocks = (rows + 3) / 4;
    hipLaunchKernelGGL(lstm_loss_rows_kernel, dim3((unsigned)nblocks), dim3(256), 0, stream,
                       (const float*)(ws + W.off_xz), S, y, w, dpre, lpart, (size_t)rows, d->T, d->F, L.Fq);
    hipLaunchKernelGGL(lstm_loss_final_kernel, dim3(1), dim3(256), 0, stream, lpart, nblocks, sums);
    return lstm_head_products(h, d, W, ws, hidden, ld_h, w_out, d_hidden, d_w_out, d_b_out, stream);
}

// include/drnmf_waveloss.h: the same head backward for a given cotangent of the sigmoid output
extern "C" int32_t drnmf_lstm_head_backward_cot(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* d_mask,
                                                int64_t ld_dm, const float* hidden, int32_t ld_h,
                                                const void* params, const float* w_out, float* d_hidden,
                                                float* d_w_out, float* d_b_out, void* workspace,
                                                size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    LstmTrainLayout W;
    int rc = validate_train_call(h, d, workspace, workspace_bytes, "lstm_head_backward_cot", &W);
    if (rc) return rc;
    if (!d_mask || !hidden || !params || !w_out || !d_hidden || !d_w_out || !d_b_out)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "lstm_head_backward_cot: NULL pointer argument");
    rc = lstm_check_ld_params(h, d, ld_h, params, "lstm_head_backward_cot");
    if (rc) return rc;
    if (ld_dm < d->F)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "lstm_head_backward_cot: ld_dm %lld < F %d", (long long)ld_dm, d->F);
    const LstmLayout& L = W.L;
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    const int64_t rows = (int64_t)d->B * d->T;
    float* S = (float*)(ws + W.off_s);
    DRNMF_HIP(h, lstm_head_product(d, L, hidden, ld_h, params, S, stream));
    hipLaunchKernelGGL(lstm_cot_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, d_mask, ld_dm,
                       (const float*)S, (float*)(ws + W.off_dpre), (size_t)rows, d->F, L.Fq);
    return lstm_head_products(h, d, W, ws, hidden, ld_h, w_out, d_hidden, d_w_out, d_b_out, stream);
}

extern "C" int32_t drnmf_lstm_backward(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* const* kernel,
                                       const float* const* recurrent, const float* d_hidden,
                                       float* const* d_kernel, float* const* d_recurrent, float* const* d_bias,
                                       void* workspace, size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    LstmTrainLayout W;
    int rc = validate_train_call(h, d, workspace, workspace_bytes, "lstm_backward", &W);
    if (rc) return rc;
    ++h->call_seq;
    if (!kernel || !recurrent || !d_hidden || !d_kernel || !d_recurrent || !d_bias)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "lstm_backward: NULL pointer argument");
    for (int k = 0; k < d->K; ++k)
        if ((k > 0 && !kernel[k]) || !recurrent[k] || !d_kernel[k] || !d_recurrent[k] || !d_bias[k])
            DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "lstm_backward: NULL pointer in the arrays (layer %d)", k);
    const LstmLayout& L = W.L;
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    float* Mt = (float*)(ws + W.off_mt);
    float* Z = (float*)(ws + W.off_z);
    float* ph = (float*)(ws + W.off_ph);
    float* pc = (float*)(ws + W.off_pc);
    int* ctr = (int*)(ws + W.off_bctr);
    const size_t layer_mt = (size_t)2 * L.NC * W.NBc;
    for (int k = 0; k < d->K; ++k) {
        const int rows = k < d->K - 1 ? 2 * L.NC : L.NC;
        const size_t tot = (size_t)rows * W.NBc;
        hipLaunchKernelGGL(lstm_pack_bwd_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream,
                           k < d->K - 1 ? kernel[k + 1] : nullptr, recurrent[k], Mt + (size_t)k * layer_mt, d->H,
                           L.NC, W.NB, rows);
    }
    const size_t nring = (size_t)d->K * 2 * L.Bp * W.NBc;
    hipLaunchKernelGGL(lstm_bwd_init_kernel, dim3((unsigned)((nring + 255) / 256)), dim3(256), 0, stream, ph, pc,
                       ctr, nring, d->T + d->K - 2);
    DRNMF_HIP(h, hipGetLastError());

    LstmBwdArgs base;
    base.Mt = Mt;
    base.Z = Z;
    base.cst = (const float*)(ws + W.off_cst);
    base.valid = (const unsigned char*)(ws + W.off_valid);
    base.dh = d_hidden;
    base.ph = ph;
    base.pc = pc;
    base.zk = W.zk;
    base.B = d->B; base.T = d->T; base.H = d->H; base.K = d->K;
    base.Bp = L.Bp; base.Hc = L.Hc; base.NB = W.NB; base.NC = L.NC;
    base.act = d->recurrent_activation;
    const dim3 grid((unsigned)W.NB, (unsigned)(L.Bp / 16), (unsigned)d->K);
    const std::vector<uint64_t> key = {
        (uint64_t)d->B, (uint64_t)d->T, (uint64_t)d->F, (uint64_t)d->H, (uint64_t)d->K,
        (uint64_t)d->recurrent_activation, (uint64_t)(uintptr_t)d_hidden, (uint64_t)(uintptr_t)workspace};
    rc = lstm_wavefront(h, stream, GraphKind::LstmBackward, key, d->T, d->K, (const void*)&lstm_bwd_step_kernel,
                        grid, base, ctr);
    if (rc) return rc;

    // time-batched weight gradients, unnormalised sums, Keras layouts
    const int64_t rows = (int64_t)d->B * (d->T + 1);
    const int H4 = 4 * d->H;
    const float* hst = (const float*)(ws + W.off_hst);
    for (int k = 0; k < d->K; ++k) {
        const float* Zk = Z + (size_t)k * W.zk * L.NC;
        // recurrent_k: sum over rows of h_{k}[row]^T dz_k[row + 1]
        DRNMF_HIP(h, lstm_tn_product(W, ws, hst + (size_t)k * W.RS * L.Hq, L.Hq, L.Hq, Zk + L.NC, L.NC, L.NC, rows,
                                     d_recurrent[k], d->H, H4, d->H, stream));
        if (k == 0)
            DRNMF_HIP(h, lstm_tn_product(W, ws, (const float*)(ws + W.off_xz), L.Fq, L.Fq, Zk, L.NC, L.NC, rows,
                                         d_kernel[0], d->F, H4, d->H, stream));
        else
            DRNMF_HIP(h, lstm_tn_product(W, ws, hst + (size_t)(k - 1) * W.RS * L.Hq, L.Hq, L.Hq, Zk, L.NC, L.NC,
                                         rows, d_kernel[k], d->H, H4, d->H, stream));
        DRNMF_HIP(h, lstm_colsum(W, ws, Zk, L.NC, L.NC, rows, d_bias[k], H4, d->H, stream));
    }
    return DRNMF_OK;
}
