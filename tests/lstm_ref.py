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


def model_forward(x, weights, K, mask_value=-1.0, recurrent_activation="hard_sigmoid"):
    """weights in Keras order (LSTMModel.get_weights) -> (sigmoid output, last hidden), fp64 numpy."""
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
