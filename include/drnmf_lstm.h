/*
 * drnmf_lstm.h -- C ABI of the LSTM baseline in libdrnmf.so: build_lstm (enhance.py:321-345), the paper's
 * comparison model,
 *     Masking(mask_value) -> LSTM(H, return_sequences=True) x K -> TimeDistributed(Dense(F))
 *                         -> TimeDistributed(Activation('sigmoid')),
 * inference and training.  Conventions as in drnmf.h: device pointers, caller-owned memory (nothing is allocated
 * inside an enqueue call), the caller's stream, the handle's mutex, never a synchronisation, status codes.
 *
 * Keras 2.0.4 LSTM semantics [K2.0.4-memory] -- Keras is not part of the reference repository:
 *   weights kernel [in][4H], recurrent_kernel [H][4H], bias [4H], gate column order i, f, c, o;
 *   z = x_t kernel + h_{t-1} recurrent_kernel + bias;
 *   i = s(z_i), f = s(z_f), c_t = f c_{t-1} + i tanh(z_c), o = s(z_o), h_t = o tanh(c_t);
 *   s = hard_sigmoid = clip(0.2 x + 0.5, 0, 1) by default (recurrent_activation), sigmoid selectable;
 *   zero initial h and c (the *_stateful entry points take and return both).
 * Masking as Theano's masked K.rnn: a frame whose bins ALL equal mask_value is masked; at a masked step the
 * output and both states are the previous step's (zeros before the first valid step), in every layer.
 */
#ifndef DRNMF_LSTM_H
#define DRNMF_LSTM_H

#include "drnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct drnmf_lstm_desc {
    int32_t B, T;                  /* sequences, frames                                              */
    int32_t F;                     /* input bins = Dense output width (enhance.py: output_dim = input_dim) */
    int32_t H;                     /* hidden_dim (units of every LSTM layer)                         */
    int32_t K;                     /* K_layers                                                       */
    int32_t recurrent_activation;  /* DRNMF_ACT_HARD_SIGMOID (Keras default) or DRNMF_ACT_SIGMOID    */
    int32_t operand_f16;           /* 0: the recurrent products contract fp32 operands (v_mfma_f32_16x16x4_f32).
                                    * 1 (extension, as drnmf_cell_desc_t.operand_f16; INFERENCE ONLY): the stacked
                                    * matrices recurrent_0 and [kernel_k; recurrent_k], k >= 1, are STORED as fp16 and
                                    * the h vectors are rounded to fp16 where they enter those products
                                    * (v_mfma_f32_16x16x32_f16, fp32 accumulation).  Everything else stays fp32:
                                    * x . kernel_0 + bias, the gates, c, the carried h, the states of the
                                    * *_stateful entry points, h_out and the head.  Conversion is the plain
                                    * round-to-nearest cast: a weight with |w| > 65504 becomes +-inf (nothing
                                    * saturates, nothing is checked).  Any other value: DRNMF_ERR_INVALID_ARG.
                                    * The training entry points return DRNMF_ERR_UNSUPPORTED for 1 (and
                                    * drnmf_lstm_train_workspace_bytes 0): train with 0 and prepare the same
                                    * weights with 1.  params and workspace sizes and layouts depend on the field:
                                    * prepare, forward and head calls must agree on it.              */
} drnmf_lstm_desc_t;

/* Prepared parameter block (B, T ignored).  Inputs in Keras layouts, float32 row-major:
 *   kernel0 [F][4H]; kernel_rest [K-1][H][4H] (NULL when K == 1); recurrent [K][H][4H]; bias [K][4H];
 *   w_out [H][F]; b_out [F].  params: 256-byte aligned, params_bytes >= drnmf_lstm_params_bytes(d)
 *   (else DRNMF_ERR_WORKSPACE). */
size_t drnmf_lstm_params_bytes(const drnmf_lstm_desc_t* d);
int32_t drnmf_lstm_prepare_params(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* kernel0,
                                  const float* kernel_rest, const float* recurrent, const float* bias,
                                  const float* w_out, const float* b_out, void* params, size_t params_bytes,
                                  void* stream);

/* Forward of the K stacked LSTM layers: x [B][T][F] -> h_out [B][T][ld_h] (the last layer's outputs in columns
 * 0 .. H-1, zeros in columns H .. ld_h-1; ld_h >= H).  ld_h = round_up(H, 4) keeps the head on its vectorised
 * path.  workspace: 256-byte aligned, >= drnmf_lstm_workspace_bytes(d) (else DRNMF_ERR_WORKSPACE). */
size_t drnmf_lstm_workspace_bytes(const drnmf_lstm_desc_t* d);
int32_t drnmf_lstm_forward(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* x, float mask_value,
                           const void* params, float* h_out, int32_t ld_h, void* workspace,
                           size_t workspace_bytes, void* stream);

/* drnmf_lstm_forward with h and c carried across calls (Keras' LSTM(stateful=True) [K2.0.4-memory]), named after
 * the cell's *_stateful entries in drnmf.h.  Every state array is [K][B][H] float32, contiguous and caller-owned
 * (layer k's state of sequence b at (k B + b) H); nothing is allocated inside the call.
 *   initial_h / initial_c: the state entering frame 0 of every layer; NULL = zeros (each on its own).
 *   final_h / final_c: the state leaving frame T-1; NULL = not wanted (nothing is written).
 * Ordering: EVERY read of initial_* happens before ANY write of final_* -- the entering state is copied into the
 * workspace by a kernel in front of the recurrence, the leaving state is copied out by one behind it -- so
 * final_x may alias initial_x (the usual call: one buffer pair carried from call to call).  Both copies run on
 * the caller's stream outside the replayed frame graphs, which therefore hold no state pointer: calls that
 * differ only in their state pointers or contents replay the same graphs.
 * Masking: a masked step copies both states, so a sequence masked for the whole call leaves with exactly the
 * state it entered with.  At masked frames BEFORE a call's first valid frame h_out is the carried h (the output
 * the previous call ended on), which makes a run cut into calls equal to the same frames run in one call.
 * [K2.0.4-memory] difference: Keras' masked K.rnn writes zeros at those frames; they carry weight 0 in every loss
 * the reference uses.  With all four pointers NULL the call computes what drnmf_lstm_forward computes, bit for
 * bit. */
int32_t drnmf_lstm_forward_stateful(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* x, float mask_value,
                                    const void* params, const float* initial_h, const float* initial_c,
                                    float* final_h, float* final_c, float* h_out, int32_t ld_h, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* Head: out [B*T][F] = sigmoid(hidden . w_out + b_out), every frame (masked ones included); hidden rows have
 * stride ld_h >= H.  With ld_h >= round_up(H, 4) the columns H .. round_up(H, 4)-1 are read and must be finite
 * (drnmf_lstm_forward writes zeros there). */
int32_t drnmf_lstm_head_forward(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* hidden, int32_t ld_h,
                                const void* params, float* out, void* stream);

/* ---- training (enhance.py:1260-1312: loss 'mse_of_masked', Adam) ----------------------------------------------
 * Three calls on ONE training workspace (256-byte aligned, >= drnmf_lstm_train_workspace_bytes(d), else
 * DRNMF_ERR_WORKSPACE), in this order:
 *
 * drnmf_lstm_train_forward: drnmf_lstm_forward (same arguments, same h_out bit for bit) that also keeps, in the
 *   workspace, the masked input and every layer's gate pre-activations, c_t and h_t for the backward.
 *
 * drnmf_lstm_loss_head_backward: sigmoid head, loss and its gradient.  xm = the Masking layer's output (x with
 *   masked frames zeroed, from the forward's workspace), s = sigmoid(hidden . w_out + b_out):
 *     per frame  loss = w * mean_F (xm * s - y)^2
 *   y [B][T][F]; w [B][T] (temporal sample weights); hidden [B][T][ld_h] = the forward's h_out; w_out [H][F]
 *   (Keras layout; the weights params was prepared from).  Outputs (overwritten, UNNORMALISED sums as
 *   drnmf_loss_head_backward): sums [2] = {sum w*loss, #frames with w != 0}; d_hidden [B][T][H];
 *   d_w_out [H][F]; d_b_out [F].
 *
 * drnmf_lstm_backward: BPTT through the K layers from d_hidden (masked frames follow K.rnn: no gradient enters
 *   them, both state gradients pass to the frame before).  kernel / recurrent: host arrays of K device pointers
 *   to the Keras weights (kernel[0] is not read); d_kernel [K] (d_kernel[0] -> [F][4H], others [H][4H]),
 *   d_recurrent [K] ([H][4H]), d_bias [K] ([4H]): host arrays of device pointers, overwritten in Keras layout with
 *   the unnormalised gradient sums. */
size_t drnmf_lstm_train_workspace_bytes(const drnmf_lstm_desc_t* d);
int32_t drnmf_lstm_train_forward(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* x, float mask_value,
                                 const void* params, float* h_out, int32_t ld_h, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* drnmf_lstm_train_forward with the state arguments of drnmf_lstm_forward_stateful (same layout, NULL rules,
 * aliasing and masking; the same h_out as drnmf_lstm_forward_stateful bit for bit).  The entering state is also
 * kept in the training workspace, in the zero frame in front of every sequence, where drnmf_lstm_backward reads
 * it: c_{t-1} of frame 0 in dz_f, h_{t-1} of frame 0 in the recurrent-kernel gradient.  It is a CONSTANT of the
 * gradient (as in drnmf_cell_backward_stateful): nothing propagates past frame 0 and no gradient with respect to
 * the state is returned -- truncated BPTT.  drnmf_lstm_loss_head_backward and drnmf_lstm_backward follow
 * unchanged; there is no backward entry point of its own. */
int32_t drnmf_lstm_train_forward_stateful(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* x,
                                          float mask_value, const void* params, const float* initial_h,
                                          const float* initial_c, float* final_h, float* final_c, float* h_out,
                                          int32_t ld_h, void* workspace, size_t workspace_bytes, void* stream);
int32_t drnmf_lstm_loss_head_backward(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* y, const float* w,
                                      const float* hidden, int32_t ld_h, const void* params, const float* w_out,
                                      float* sums, float* d_hidden, float* d_w_out, float* d_b_out, void* workspace,
                                      size_t workspace_bytes, void* stream);
int32_t drnmf_lstm_backward(drnmf_handle_t h, const drnmf_lstm_desc_t* d, const float* const* kernel,
                            const float* const* recurrent, const float* d_hidden, float* const* d_kernel,
                            float* const* d_recurrent, float* const* d_bias, void* workspace,
                            size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRNMF_LSTM_H */
