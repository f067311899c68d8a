"""numpy fp64 emulation of the LSTM baseline with operand_f16 (csrc/lstm.hip, lstm_step_kernel<false, true>): it is
lstm_ref.lstm_layers with the operands of the recurrent products rounded to fp16 first.

Rounded (round-to-nearest _Float16, numpy's float16 cast): the stacked matrices recurrent_0 (layer 0) and
[kernel_k; recurrent_k] (k >= 1), and the h vectors entering those products, h_{k-1,t} and h_{k,t-1}.
Unrounded: x . kernel_0 + bias, the gates, c, the carried h (a masked step copies the unrounded h), the head
(lstm_ref.head).

accumulate: 'fp64' sums the products of the rounded operands exactly (to fp64); 'fp32chunk' sums them in float32
in 32-row chunks of each operand half, the chunks added one after another in float32 -- ONE float32 order among
many (the device's is another: four waves take every fourth chunk, the matrix core sums 32 products at a time,
LDS adds the four partials).  The distance between the two settings measures what the accumulation order is worth.

Also the table of the shapes tests/test_gpu_lstm_f16.py runs and the constants tests/test_lstm_f16_host.py
records for them, shared by both files.
"""
import functools

import numpy as np
import torch

import lstm_ref as R
import lstm_state_ref as SR


def f16(a):
    """fp64 value of the nearest _Float16."""
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def _act(name):
    if name == "sigmoid":
        return lambda v: 1.0 / (1.0 + np.exp(-v))
    if name == "hard_sigmoid":
        return lambda v: np.clip(0.2 * v + 0.5, 0.0, 1.0)
    raise ValueError(name)


def _products(pairs, accumulate):
    """sum over (h, W) pairs of f16(h) @ f16(W); h [B,R], W [R,4H]."""
    if accumulate == "fp64":
        return sum(f16(h) @ f16(W) for h, W in pairs)
    if accumulate != "fp32chunk":
        raise ValueError(accumulate)
    acc = None
    for h, W in pairs:
        h32, W32 = f16(h).astype(np.float32), f16(W).astype(np.float32)
        for r0 in range(0, h32.shape[1], 32):
            part = h32[:, r0:r0 + 32] @ W32[r0:r0 + 32]
            acc = part if acc is None else (acc + part).astype(np.float32)
    return acc.astype(np.float64)


def lstm_layers(x, kernels, recurrents, biases, mask_value=-1.0, recurrent_activation="hard_sigmoid",
                accumulate="fp64", state=None):
    """x [B,T,F]; Keras-layout weights per layer -> (list of every layer's outputs [B,T,H], (h, c) leaving the last
    frame, each [K,B,H]); fp64 numpy.  state: the (h, c) entering frame 0, each [K,B,H] (None: zeros)."""
    x = np.asarray(x, dtype=np.float64)
    sig = _act(recurrent_activation)
    m = R.valid_frames(x, mask_value).numpy()[..., None]
    inp = x * m
    B, T, _ = x.shape
    outs, fin_h, fin_c = [], [], []
    for k, (W, U, b) in enumerate(zip(kernels, recurrents, biases)):
        W, U, b = (np.asarray(v, dtype=np.float64) for v in (W, U, b))
        H = U.shape[0]
        h = np.zeros((B, H)) if state is None else np.array(state[0][k], dtype=np.float64)
        c = np.zeros((B, H)) if state is None else np.array(state[1][k], dtype=np.float64)
        seq = []
        for t in range(T):
            if k == 0:
                z = inp[:, t] @ W + b + _products([(h, U)], accumulate)
            else:
                z = b + _products([(inp[:, t], W), (h, U)], accumulate)
            i, f, g, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
            cn = sig(f) * c + sig(i) * np.tanh(g)
            hn = sig(o) * np.tanh(cn)
            v = m[:, t]
            c = np.where(v, cn, c)
            h = np.where(v, hn, h)
            seq.append(h)
        out = np.stack(seq, axis=1)
        outs.append(out)
        fin_h.append(h)
        fin_c.append(c)
        inp = out
    return outs, (np.stack(fin_h), np.stack(fin_c))


def model_forward(x, weights, K, mask_value=-1.0, recurrent_activation="hard_sigmoid", accumulate="fp64",
                  state=None):
    """weights in Keras order (LSTMModel.get_weights) -> (sigmoid output, last hidden, leaving (h, c))."""
    ks, rs, bs = weights[0:3 * K:3], weights[1:3 * K:3], weights[2:3 * K:3]
    hs, fin = lstm_layers(x, ks, rs, bs, mask_value, recurrent_activation, accumulate, state)
    y = R.head(torch.from_numpy(hs[-1]), weights[3 * K], weights[3 * K + 1]).numpy()
    return y, hs[-1], fin


def rel(got, ref):
    """max|d| / max|ref|"""
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref))) / max(float(np.max(np.abs(ref))), 1e-30)


# ---- the GPU test's cases -------------------------------------------------------------------------------------
# (B, T, F, H, K), the smallest shapes that reach each branch of the fp16 step kernel:
#   (1, 1, 5, 13, 1)    single chunk, padded units, layer-0-only path
#   (3, 2, 9, 13, 3)    K > T, diagonals with dead pairs
#   (17, 9, 33, 54, 2)  two row blocks with padded rows, Hc = 64, 7 unit tiles with the last padded
#   (5, 7, 33, 70, 3)   nch = 3 and 6: not a multiple of the wave count, so the clamped path
#   (4, 6, 17, 32, 2)   H exactly one chunk, no padding
# input: 'ragged' = lstm_ref.ragged_input (valid prefixes; its all-masked row where B > 1), 'mixed' =
# lstm_ref.masked_input(pattern="mixed") (interior masks).  scale: random_weights(scale=), large enough per case
# for the reference condition of tests/test_lstm_f16_host.py (the fp16 rounding must show in the head output).
D_F32 = 1e-4        # TOL of tests/test_gpu_lstm.py: what the fp32 kernels are held to against the fp64 reference


class Case(object):
    def __init__(self, shape, act, inp, scale, seed, d_acc, state=False):
        self.shape, self.act, self.inp, self.scale, self.seed, self.d_acc = shape, act, inp, scale, seed, d_acc
        self.state = state          # True: a non-zero (h, c) enters frame 0 (lstm_state_ref.random_state)
        self.id = "B%dT%dF%dH%dK%d-%s-%s" % (shape + (act, inp))

    @property
    def tol_emu(self):
        """The tight bound: 4 * max(D_acc, D_f32); the 4 covers the device's accumulation order, which is neither
        emulation's."""
        return 4 * max(self.d_acc, D_F32)


# d_acc: the recorded upper bound of D_acc (test_lstm_f16_host.py asserts that the measured value stays under it).
# Beside each case the measured D_acc / D_f16 (head output, max|d| / max|ref|).  D_acc is not an fp32 rounding
# level: where the two accumulation orders leave an h on different sides of an fp16 rounding boundary, one operand
# moves by a whole fp16 ulp, and that is what the figures of 1e-5 and more are.
# state=True: a non-zero (h, c) enters frame 0.  (1, 1, 5, 13, 1) needs it -- from the zero state its only recurrent
# product is zero and D_f16 with it -- and it needs large weights: the rounding error of h . recurrent_0 is
# absolute, and shows once that product is large and mostly cancelled by x . kernel_0 + bias.  The largest weight
# is 337, far inside the fp16 range.
CASES = [
    Case((1, 1, 5, 13, 1), "hard_sigmoid", "ragged", 256.0, 21, 1e-6, state=True),  # 3.5e-07 / 3.62e-03
    Case((3, 2, 9, 13, 3), "hard_sigmoid", "mixed", 16.0, 9, 1e-7),                # 5.2e-08 / 2.53e-03
    Case((17, 9, 33, 54, 2), "hard_sigmoid", "ragged", 6.0, 4, 3e-5),              # 2.3e-05 / 2.03e-03
    Case((17, 9, 33, 54, 2), "sigmoid", "mixed", 6.0, 0, 1e-6),                    # 4.4e-07 / 2.47e-03
    Case((5, 7, 33, 70, 3), "hard_sigmoid", "mixed", 6.0, 2, 1e-5),                # 5.5e-06 / 2.90e-03
    Case((5, 7, 33, 70, 3), "sigmoid", "ragged", 6.0, 5, 3e-5),                    # 1.6e-05 / 1.67e-03
    Case((4, 6, 17, 32, 2), "hard_sigmoid", "ragged", 6.0, 3, 1e-7),               # 5.4e-08 / 2.89e-03
]


def case_inputs(cs):
    """(x, weights, entering state or None) of a case, from its seed."""
    B, T, F, H, K = cs.shape
    rng = np.random.default_rng(cs.seed)
    w = R.random_weights(rng, F, H, K, scale=cs.scale)
    if cs.inp == "ragged":
        x, _ = R.ragged_input(rng, B, T, F)
    else:
        x, _ = R.masked_input(rng, B, T, F, "mixed")
    st = SR.random_state(rng, K, B, H) if cs.state else None
    return x, w, st


@functools.lru_cache(maxsize=None)
def case_data(i):
    """(x, weights, state, y_emu, h_emu, y_exact) of CASES[i]: computed once, shared by the tests, never written
    to.  y_emu / h_emu: the fp64-accumulate emulation; y_exact: the unrounded reference."""
    cs = CASES[i]
    x, w, st = case_inputs(cs)
    K = cs.shape[4]
    y_emu, h_emu, _ = model_forward(x, w, K, -1.0, cs.act, "fp64", st)
    y_exact = SR.model_forward(x, w, K, -1.0, cs.act, st)[0]
    for a in (x, y_emu, h_emu, y_exact) + tuple(w) + (st or ()):
        a.setflags(write=False)
    return x, w, st, y_emu, h_emu, y_exact
