// Host side of the recurrent cell, shared by its forward drivers (cell_forward.hip) and its BPTT
// (cell_backward.hip): one call's forward workspace and prepared parameter block as typed views.
// No device code.  Include after cell_shared.h (Workspace, ParamsLayout).  Built in place:
//     CellCtx C{*d, W, params_layout(d), (char*)workspace, (const char*)params};
#pragma once

namespace {

// a float as a field of a graph key
static inline uint64_t f32_bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
// frames per graph: `nodes` kernel nodes at `per_frame` launches a frame; 1 .. 64, at most T
static inline int frames_per_graph(int nodes, int per_frame, int T) {
    const int n = nodes / per_frame < 1 ? 1 : (nodes / per_frame > 64 ? 64 : nodes / per_frame);
    return n > T ? T : n;
}

struct CellCtx {
    drnmf_cell_desc_t d;
    Workspace W;
    ParamsLayout L;
    char* ws;            // the forward workspace (of a sub-batch: its own slice)
    const char* pb;      // the prepared block (drnmf_prepare_params)
    bool half = d.operand_f16 != 0;      // the forward runs on fp16 matrix-core operands

    // ---- forward workspace (workspace_layout) ----------------------------------------------------
    float* xp = (float*)(ws + W.off_xp);                     // packed input of every frame
    f16* xp16 = half ? (f16*)(ws + W.off_xp16) : nullptr;    // fp16 mode: once more as fp16
    unsigned char* valid = (unsigned char*)(ws + W.off_valid);
    unsigned char* seen = (unsigned char*)(ws + W.off_seen);
    float* psum_all = (float*)(ws + W.off_psum_all);
    float* rpart = (float*)(ws + W.off_rpart);
    float* hb[2] = {(float*)(ws + W.off_h0), (float*)(ws + W.off_h1)};
    f16* hb16[2] = {(f16*)(ws + W.off_h16_0), (f16*)(ws + W.off_h16_1)};     // fp16 mode: Hp16 ping-pong
    f16* r16 = (f16*)(ws + W.off_r16);                                        // ... and Rp16
    float* state = (float*)(ws + W.off_state);
    float* rs_part = (float*)(ws + W.off_rs);
    float* psum = (float*)(ws + W.off_psum);
    float* qpart = (float*)(ws + W.off_qpart);               // odd-bin side path
    float* qsum = (float*)(ws + W.off_qsum);
    float* xtail = (float*)(ws + W.off_xtail);
    float* xcur = (float*)(ws + W.off_xcur);
    int* tA = (int*)(ws + W.off_t);      // frame index read by every kernel of a frame
    int* tB = tA + 16;                   // next frame index, published by the last kernel
    unsigned* bar = (unsigned*)(ws + W.off_t + 256);         // the persistent chains' sync lines
    float* Cp = (float*)(ws + W.off_cp);                     // Gram form: hoisted c_k,
    float* xpad = (float*)(ws + W.off_xpad);                 // one block of padded x,
    float* qb[2] = {(float*)(ws + W.off_q0), (float*)(ws + W.off_q1)};       // q ping-pong
    float* rsave = W.off_rsave ? (float*)(ws + W.off_rsave) : nullptr;       // saved residuals; NULL = absent
    // relu sign bits of the stored hiddens (cell_shared.h); NULL = absent, or switched off for this call.  The
    // forward that records them and the BPTT that reads them decide alike: same layout, same variable
    unsigned* relu_bits = (W.off_bits && relu_bits_wanted()) ? (unsigned*)(ws + W.off_bits) : nullptr;
    float* xhat = W.off_xhat ? (float*)(ws + W.off_xhat) : nullptr;          // KL / beta training: x^; NULL = absent

    // ---- prepared block (params_layout), per layer -----------------------------------------------
    // Quantities derived from the dictionary are stored once per STORED layer: a tied dictionary
    // (n_D == 1) serves every layer from slot 0.  inv_alpha and bias are kept per layer always.
    size_t stored(int k, size_t stride) const { return d.n_D == 1 ? 0 : (size_t)k * stride; }
    size_t dstride() const { return (size_t)L.Fp * L.Np; }
    const float* ia_of(int k) const { return (const float*)(pb + L.off_inv_alpha) + (size_t)k * L.Np; }
    const float* b_of(int k) const { return (const float*)(pb + L.off_bias) + (size_t)k * L.Np; }
    const float* tail_of(int k) const {
        return (const float*)(pb + L.off_tail) + stored(k, (size_t)MAX_TAIL * L.Np);
    }
    // fp32 packings: cell_b's (Dp) and cell_a's / bwd_a's (DpA).  A block prepared for fp16 operands
    // keeps both behind each other at off_dn32, for the fp32 BPTT.
    const float* Dp_of(int k) const {
        return (const float*)(pb + (half ? L.off_dn32 : L.off_dn)) + stored(k, dstride());
    }
    const float* DpA_of(int k) const {
        return (half ? Dp_of(0) + (size_t)d.n_D * dstride() : (const float*)(pb + L.off_dnA)) + stored(k, dstride());
    }
    // the forward's operands: the fp32 packings, or the ONE fp16 packing both kernels read (never the KL / beta
    // cell's: validate_cell_desc refuses operand_f16 there)
    const char* Dn_of(int k) const {
        return half ? pb + L.off_dn + stored(k, dstride() * 2) : (const char*)Dp_of(k);
    }
    const char* DnA_of(int k) const { return half ? Dn_of(k) : (const char*)DpA_of(k); }
    // Gram form
    size_t g_stride() const { return stored(1, (size_t)L.Np * L.Np); }
    const float* G_of(int k) const { return (const float*)(pb + L.off_gram) + (size_t)k * g_stride(); }
    const float* DnT_of(int k) const { return (const float*)(pb + L.off_dnT) + stored(k, (size_t)L.Np * L.Fp); }
};

}  // namespace
