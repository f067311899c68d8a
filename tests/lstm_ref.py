"""fp64 torch restatement of build_lstm (enhance.py:321-345) -- the contract csrc/lstm.hip implements.

Keras 2.0.4 LSTM [K2.0.4-memory]: z = x_t kernel + h_{t-1} recurrent_kernel + bias, gate columns i, f, c, o;
i = s(z_i), f = s(z_f), c_t = f c_{t-1} + i tanh(z_c), o = s(z_o), h_t = o tanh(c_t); s = hard_sigmoid
(clip(0.2 x + 0.5, 0, 1)) or sigmoid; zero initial states.  Masking as Theano's masked K.rnn: a frame whose
bins all equal mask_value is masked; there the output and both states are the previous step's, in every layer.
Head: sigmoid(h . W_out + b_out) on every frame.  Differentiable (torch autograd), no GPU needed.
"""
import numpy as np
import torch


def _act(name):
    if name == "sigmoid":
        return torch.sigmoid
    if name == "hard_sigmoid":
        return lambda v: torch.clamp(0.2 * v + 0.5, 0.0, 1.0)
    raise ValueError(name)


def valid_frames(x, mask_value):
    """[B,T] bool: False where every bin equals mask_value (keras Masking)."""
    x = torch.as_tensor(np.asarray(x)) if not isinstance(x, torch.Tensor) else x
    if mask_value is None:
        return torch.ones(x.shape[:2], dtype=torch.bool)
    return (x != mask_value).any(dim=-1)


def lstm_layers(x, kernels, recurrents, biases, mask_value=-1.0, recurrent_activation="hard_sigmoid"):
    """x [B,T,F]; per layer kernel [in,4H], recurrent_kernel [H,4H], bias [4H] -> list of every layer's
    outputs [B,T,H] (fp64 torch tensors)."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float64)) if not isinstance(x, torch.Tensor) else x.double()
    sig = _act(recurrent_activation)
    m = valid_frames(x, mask_value).unsqueeze(-1)
    inp = x * m                                   # Masking zeroes masked frames
    B, T, _ = x.shape
    outs = []
    for W, U, b in zip(kernels, recurrents, biases):
        W, U, b = (torch.as_tensor(np.asarray(v, dtype=np.float64)) if not isinstance(v, torch.Tensor)
                   else v.double() for v in (W, U, b))
        H = U.shape[0]
        h = torch.zeros(B, H, dtype=torch.float64)
        c = torch.zeros(B, H, dtype=torch.float64)
        seq = []
        for t in range(T):
            z = inp[:, t] @ W + h @ U + b
            i, f, g, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
            cn = sig(f) * c + sig(i) * torch.tanh(g)
            hn = sig(o) * torch.tanh(cn)
            v = m[:, t]
            c = torch.where(v, cn, c)
            h = torch.where(v, hn, h)
            seq.append(h)
        out = torch.stack(seq, dim=1)
        outs.append(out)
        inp = out
    return outs


def head(h, w_out, b_out):
    w_out = torch.as_tensor(np.asarray(w_out, dtype=np.float64)) if not isinstance(w_out, torch.Tensor) \
        else w_out.double()
    b_out = torch.as_tensor(np.asarray(b_out, dtype=np.float64)) if not isinstance(b_out, torch.Tensor) \
        else b_out.double()
    return torch.sigmoid(h @ w_out + b_out)


def model_forward(x, weights, K, mask_value=-1.0, recurrent_activation="hard_sigmoid", rows=None):
    """weights in Keras order (LSTMModel.get_weights) -> (sigmoid output, last hidden), fp64 numpy.  rows: the
    sequences to run (an index list into x's first axis; rows never interact), outputs in that order."""
    if rows is not None:
        x = x[torch.as_tensor(list(rows))] if isinstance(x, torch.Tensor) else np.asarray(x)[list(rows)]
    ks, rs, bs = weights[0:3 * K:3], weights[1:3 * K:3], weights[2:3 * K:3]
    hs = lstm_layers(x, ks, rs, bs, mask_value, recurrent_activation)
    y = head(hs[-1], weights[3 * K], weights[3 * K + 1])
    return y.numpy(), hs[-1].numpy()


def random_weights(rng, F, H, K, scale=1.0):
    """Keras-layout weights large enough that both gate nonlinearities leave their linear range."""
    w = []
    for k in range(K):
        fin = F if k == 0 else H
        w += [(rng.standard_normal((fin, 4 * H)) * scale / np.sqrt(fin)).astype(np.float32),
              (rng.standard_normal((H, 4 * H)) * scale / np.sqrt(H)).astype(np.float32),
              (0.3 * rng.standard_normal(4 * H)).astype(np.float32)]
    w += [(rng.standard_normal((H, F)) / np.sqrt(H)).astype(np.float32),
          (0.1 * rng.standard_normal(F)).astype(np.float32)]
    return w


def ragged_input(rng, B, T, F, mask_value=-1.0, all_masked_row=True):
    """x [B,T,F] float32 with ragged valid prefixes padded by mask_value (one row fully masked, one full)."""
    x = rng.random((B, T, F)).astype(np.float32)
    lens = rng.integers(1, T + 1, size=B)
    lens[0] = T
    if all_masked_row and B > 1:
        lens[-1] = 0
    for b in range(B):
        x[b, lens[b]:] = mask_value
    return x, lens


MASK_PATTERNS = ("none", "trailing", "leading", "interior", "partial", "all", "combo")


def masked_input(rng, B, T, F, pattern="mixed", mask_value=-1.0):
    """x [B,T,F] float32 and the frame validity it was built with, valid [B,T] bool (independent of
    valid_frames).  Valid frames hold bins in (0, 1] with about one bin in ten set to mask_value (a valid frame
    may contain the mask value; silence in a magnitude spectrogram is 0); a masked frame holds mask_value in
    every bin.  pattern, per row (one of MASK_PATTERNS, or 'mixed': row b takes MASK_PATTERNS[b % 7]):
      none      every frame valid
      trailing  a masked suffix (the reference's padding layout)
      leading   a masked prefix (the states stay zero until the first valid frame)
      interior  one or two masked runs strictly inside the sequence (the states carry across them)
      partial   about a third of the frames have every bin but one equal to mask_value (still valid; the
                surviving bin is never bin 0 when F > 1)
      all       every frame masked
      combo     a masked prefix, an interior run, partial frames and a masked suffix in one row"""
    mv = np.float32(mask_value)
    x = (1.0 - rng.random((B, T, F))).astype(np.float32)
    x[rng.random((B, T, F)) < 0.1] = mv
    valid = np.ones((B, T), dtype=bool)

    def run(lo, hi):
        return (int(lo), int(max(lo, hi)))

    for b in range(B):
        kind = MASK_PATTERNS[b % len(MASK_PATTERNS)] if pattern == "mixed" else pattern
        if kind not in MASK_PATTERNS:
            raise ValueError(pattern)
        masked, partial = [], []
        if kind == "all":
            masked.append((0, T))
        if kind in ("trailing", "combo") and T > 1:
            masked.append(run(T - rng.integers(1, max(2, T // 4 + 1)), T))
        if kind in ("leading", "combo") and T > 1:
            masked.append(run(0, rng.integers(1, max(2, T // 4 + 1))))
        if kind in ("interior", "combo") and T > 2:
            lo, hi = T // 4 + 1, max(T // 4 + 2, 3 * T // 4)
            a = int(rng.integers(lo, hi)) if hi > lo else lo
            a = min(a, T - 2)
            masked.append(run(a, min(T - 1, a + 1 + rng.integers(0, max(1, T // 8)))))
            if kind == "interior" and T > 6 and a > 2:            # a second run, before the first
                masked.append(run(1, 2))
        if kind in ("partial", "combo"):
            partial = [t for t in range(T) if rng.random() < 1 / 3]
        for lo, hi in masked:
            x[b, lo:hi] = mv
            valid[b, lo:hi] = False
        for t in partial:
            if not valid[b, t]:
                continue
            keep = int(rng.integers(1, F)) if F > 1 else 0
            x[b, t] = mv
            x[b, t, keep] = 1.0 - rng.random()
    lost = valid & (x == mv).all(axis=-1)            # a valid frame that the sprinkled mask values covered
    x[lost, -1] = 0.5
    return x, valid
