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
#include "common.h"
#include "gemm_nt.h"
#include "../../include/drnmf_lstm.h"

namespace {

// Gate-interleaved packing of the 4H gate columns: output tile ab (32 columns) holds the gates i, f, c, o of
// the 8 units 8 ab .. 8 ab + 7, column 8 g + u = gate g of unit 8 ab + u.  The workgroup that contracts a tile
// then owns everything the cell update of its 16 rows x 8 units needs: c_t and h_t are formed from registers
// and LDS, no gate values go through memory.
constexpr int LSTM_UNITS = 8;
constexpr int LSTM_NW = 4;     // waves per workgroup (the contraction split over them, reduced through LDS)
constexpr int LSTM_G = 4;      // 16-row chunks in flight per wave

struct LstmLayout {
    int Bp, Hc, Hq, Fq, numU, NC;
    size_t off_bias, off_k0t, off_wo, off_bo, params_total;
    size_t off_xz, off_valid, off_xproj, off_h, off_c, off_ctr, ws_total;
    // floats before layer k's stacked matrix: layer 0 has Hc rows (recurrent_0), layers k >= 1 have 2 Hc
    size_t m_floats(int k) const { return k == 0 ? 0 : (size_t)Hc * NC * (2 * k - 1); }
};

LstmLayout lstm_layout(const drnmf_lstm_desc_t* d) {
    LstmLayout L;
    L.Bp = pad_b(d->B > 0 ? d->B : 1);
    L.Hc = round_up(d->H, 16);             // activation width: whole 16-row chunks of the contraction
    L.Hq = round_up(d->H, 4);
    L.Fq = round_up(d->F, 4);              // xz / kernel_0^T rows: 16-byte loads in the gemm
    L.numU = (d->H + LSTM_UNITS - 1) / LSTM_UNITS;
    L.NC = L.numU * 32;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += round_up_sz(bytes, 256); return at; };
    take(L.m_floats(d->K) * 4);
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

// zero initial h and c of every layer (both ring slots, padding included), diagonal counters = 0
__global__ void __launch_bounds__(256)
lstm_init_kernel(float* __restrict__ hring, float* __restrict__ cring, int* ctr, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) { ctr[0] = 0; ctr[16] = 0; }
    if (i < n) { hring[i] = 0.f; cring[i] = 0.f; }
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
};

// One launch = one diagonal d: workgroup (ab, mb, k) computes frame t = d - k of layer k for rows
// 16 mb .. 16 mb + 15 and units 8 ab .. 8 ab + 7 (exits at once when t is out of range).  Exact-fp32 MFMA
// (v_mfma_f32_16x16x4_f32) over the contraction, split over the waves and reduced through LDS as in
// dense_step_kernel; the activations are read row-major -- lane (q, row j) takes h[j][16 c + 4 q .. + 3] as one
// 16-byte piece, which is the order the matrix packing puts the rows in.  Ring slots: (k, t) writes slot
// t & 1 of layer k; in the same launch (k + 1, t - 1) and (k, t) read slot (t - 1) & 1 of layer k, and (k, t)
// reads slot t & 1 of layer k - 1, which (k - 1, t + 1) does not write (it writes slot (t + 1) & 1).
__global__ void __launch_bounds__(64 * LSTM_NW) lstm_step_kernel(const LstmStepArgs a) {
    __shared__ __attribute__((aligned(16))) float red[LSTM_NW * 16 * 32];
    const int ab = blockIdx.x, mb = blockIdx.y, k = blockIdx.z;
    const int d = *a.d_rd;
    if (ab == 0 && mb == 0 && k == 0 && threadIdx.x == 0) *a.d_wr = d + 1;
    const int t = d - k;
    if (t < 0 || t >= a.T) return;
    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63, j = l & 15, q = l >> 4;
    const int Hc = a.Hc, nh = Hc / 16, nch = k == 0 ? nh : 2 * nh;
    const size_t slab = (size_t)a.Bp * Hc;
    const size_t arow = (size_t)(mb * 16 + j) * Hc + 4 * q;
    const float* prev = a.hring + ((size_t)k * 2 + ((t + 1) & 1)) * slab + arow;                 // h_{k,t-1}
    const float* below = k > 0 ? a.hring + ((size_t)(k - 1) * 2 + (t & 1)) * slab + arow : prev;  // h_{k-1,t}
    const size_t m_off = k == 0 ? 0 : (size_t)Hc * a.NC * (2 * k - 1);
    const float* brow = a.M + m_off + (size_t)ab * 512 + l * 4;
    const size_t bstep = (size_t)a.numU * 512;

    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
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
    const bool real = b < a.B;
    if (n >= a.H) {                                     // padded units stay zero (they meet zero matrix rows)
        if (k == a.K - 1 && real && n < a.ld_h) a.out[frame * a.ld_h + n] = 0.f;
        return;
    }
    const float* pre = k == 0 ? a.xproj + (real ? frame : 0) * a.NC : a.bias + (size_t)k * a.NC;
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
    if (real && a.valid[frame]) {
        const float ig = gate_act(z[0], a.act), fg = gate_act(z[1], a.act), og = gate_act(z[3], a.act);
        cn = fg * cn + ig * tanhf(z[2]);
        hn = og * tanhf(cn);
    }
    a.cring[e_cur] = cn;
    a.hring[e_cur] = hn;
    if (k == a.K - 1 && real) a.out[frame * a.ld_h + n] = hn;
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
        hipLaunchKernelGGL(lstm_pack_step_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream,
                           k == 0 ? nullptr : kernel_rest + (size_t)(k - 1) * HH4, recurrent + (size_t)k * HH4,
                           (float*)base + L.m_floats(k), d->H, L.Hc, L.numU, rows);
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

extern "C" int32_t drnmf_lstm_forward(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* x,
                                      float mask_value, const void* params, float* h_out, int32_t ld_h,
                                      void* workspace,
                                      size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    int rc = validate_lstm_desc(h, d, true);
    if (rc) return rc;
    ++h->call_seq;                   // (a top-level call: the graphs it takes are pinned until it returns)
    if (!x || !params || !h_out || !workspace)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "lstm_forward: NULL pointer argument");
    if (ld_h < d->H) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "lstm_forward: ld_h %d < H %d", ld_h, d->H);
    const LstmLayout L = lstm_layout(d);
    if (workspace_bytes < L.ws_total)
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "lstm_forward: workspace %zu < required %zu", workspace_bytes,
                   L.ws_total);
    if (((uintptr_t)workspace & 255) || ((uintptr_t)params & 255))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "workspace/params must be 256-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    const char* pb = (const char*)params;
    float* xz = (float*)(ws + L.off_xz);
    unsigned char* valid = (unsigned char*)(ws + L.off_valid);
    float* xproj = (float*)(ws + L.off_xproj);
    float* hring = (float*)(ws + L.off_h);
    float* cring = (float*)(ws + L.off_c);
    int* ctr = (int*)(ws + L.off_ctr);
    const size_t rows = (size_t)d->B * d->T;

    hipLaunchKernelGGL(lstm_pack_x_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, x, xz, valid,
                       mask_value, rows, d->F, L.Fq);
    const size_t nring = (size_t)d->K * 2 * L.Bp * L.Hc;
    hipLaunchKernelGGL(lstm_init_kernel, dim3((unsigned)((nring + 255) / 256)), dim3(256), 0, stream, hring,
                       cring, ctr, nring);
    DRNMF_HIP(h, hipGetLastError());
    {
        gemm::Operands g;
        g.A = xz;
        g.Bt = (const float*)(pb + L.off_k0t);
        g.M = (int64_t)rows;
        g.N = L.NC;
        g.K = L.Fq;
        g.lda = g.ldb = L.Fq;
        DRNMF_HIP(h, gemm::launch(g, EpiLstmXproj{xproj, (const float*)(pb + L.off_bias), L.NC}, stream));
    }

    LstmStepArgs base;
    base.M = (const float*)pb;
    base.bias = (const float*)(pb + L.off_bias);
    base.xproj = xproj;
    base.valid = valid;
    base.hring = hring;
    base.cring = cring;
    base.out = h_out;
    base.B = d->B; base.T = d->T; base.H = d->H; base.K = d->K;
    base.Bp = L.Bp; base.Hc = L.Hc; base.numU = L.numU; base.NC = L.NC;
    base.act = d->recurrent_activation;
    base.ld_h = ld_h;
    const dim3 grid((unsigned)L.numU, (unsigned)(L.Bp / 16), (unsigned)d->K);
    // one graph frame = two diagonals: the first reads counter 0 and sets counter 1, the second the other way
    // round (nobody reads a counter in the launch that writes it).  An odd diagonal count ends on one launch
    // whose workgroups all exit at once.
    auto frame = [&](Launcher& chain, int) -> int32_t {
        for (int p = 0; p < 2; ++p) {
            LstmStepArgs a = base;
            a.d_rd = ctr + 16 * p;
            a.d_wr = ctr + 16 * (1 - p);
            void* kp[1] = {&a};
            DRNMF_HIP(h, chain.add((const void*)&lstm_step_kernel, grid, dim3(64 * LSTM_NW), kp));
        }
        return DRNMF_OK;
    };
    const int diagonals = d->T + d->K - 1, frames = (diagonals + 1) / 2;
    const int fpg = frames < 64 ? frames : 64;
    const std::vector<uint64_t> key = {
        (uint64_t)d->B, (uint64_t)d->T, (uint64_t)d->F, (uint64_t)d->H, (uint64_t)d->K,
        (uint64_t)d->recurrent_activation, (uint64_t)(uintptr_t)params, (uint64_t)(uintptr_t)h_out, (uint64_t)ld_h,
        (uint64_t)(uintptr_t)workspace};
    return replay_frames(h, stream, GraphKind::Lstm, key, {fpg, 1}, 0, frames, frame);
}

// With ld_h >= round_up(H, 4) the product contracts the padding columns too (against zero rows of W_out^T): K and
// lda are then multiples of 4 and the gemm takes its vectorised path (and the split-operand one in bf16x3 mode).
extern "C" int32_t drnmf_lstm_head_forward(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* hidden,
                                           int32_t ld_h, const void* params, float* out, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    int rc = validate_lstm_desc(h, d, true);
    if (rc) return rc;
    if (!hidden || !params || !out) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "lstm_head_forward: NULL pointer argument");
    if (ld_h < d->H) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "lstm_head_forward: ld_h %d < H %d", ld_h, d->H);
    if ((uintptr_t)params & 255) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "params must be 256-byte aligned");
    const LstmLayout L = lstm_layout(d);
    const char* pb = (const char*)params;
    gemm::Operands g;
    g.A = hidden;
    g.Bt = (const float*)(pb + L.off_wo);
    g.M = (int64_t)d->B * d->T;
    g.N = d->F;
    g.K = ld_h >= L.Hq ? L.Hq : d->H;
    g.lda = ld_h;
    g.ldb = L.Hq;
    DRNMF_HIP(h, gemm::launch(g, EpiLstmHead{out, (const float*)(pb + L.off_bo), d->F}, (hipStream_t)stream_));
    return DRNMF_OK;
}
