"""fp64 torch reference of the LSTM baseline with h and c carried across calls (Keras' LSTM(stateful=True)
[K2.0.4-memory]; the contract of drnmf_lstm_forward_stateful / drnmf_lstm_train_forward_stateful), built next to
tests/lstm_ref.py: the same cell, the same masking, plus a state [K,B,H] entering frame 0 of every layer and the
state leaving frame T-1.  A masked step copies both states and the output, so at masked frames before a call's
first valid frame the output is the CARRIED h (Keras would write zeros there): a run cut into calls equals the
same frames run in one call.  The training loss takes the entering state as a constant (detached): truncated
BPTT.  Differentiable with torch autograd; no GPU needed.
"""
import numpy as np
import torch

import lstm_ref as R


def _t64(v):
    return v.double() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, dtype=np.float64))


def lstm_layers(x, kernels, recurrents, biases, mask_value=-1.0, recurrent_activation="hard_sigmoid",
                initial_h=None, initial_c=None):
    """lstm_ref.lstm_layers with an entering state: initial_h / initial_c [K,B,H] (None: zeros), taken as
    constants.  Returns (every layer's outputs [B,T,H], final_h [K,B,H], final_c [K,B,H]), fp64 torch."""
    x = _t64(x)
    sig = R._act(recurrent_activation)
    m = R.valid_frames(x, mask_value).unsqueeze(-1)
    inp = x * m
    B, T, _ = x.shape
    outs, fh, fc = [], [], []
    for k, (W, U, b) in enumerate(zip(kernels, recurrents, biases)):
        W, U, b = _t64(W), _t64(U), _t64(b)
        H = U.shape[0]
        h = torch.zeros(B, H, dtype=torch.float64) if initial_h is None else _t64(initial_h)[k].detach()
        c = torch.zeros(B, H, dtype=torch.float64) if initial_c is None else _t64(initial_c)[k].detach()
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
        fh.append(h)
        fc.append(c)
        inp = out
    return outs, torch.stack(fh), torch.stack(fc)


def model_forward(x, weights, K, mask_value=-1.0, recurrent_activation="hard_sigmoid", state=None):
    """weights in Keras order; state = (h, c) [K,B,H] or None -> (sigmoid output, last hidden, (final_h, final_c)),
    fp64 numpy."""
    ks, rs, bs = weights[0:3 * K:3], weights[1:3 * K:3], weights[2:3 * K:3]
    ih, ic = state if state is not None else (None, None)
    hs, fh, fc = lstm_layers(x, ks, rs, bs, mask_value, recurrent_activation, ih, ic)
    y = R.head(hs[-1], weights[3 * K], weights[3 * K + 1])
    return y.numpy(), hs[-1].numpy(), (fh.numpy(), fc.numpy())


def chunked_forward(x, cuts, weights, K, mask_value=-1.0, recurrent_activation="hard_sigmoid", state=None):
    """x cut along T into pieces of lengths `cuts`, each run from the state the one before left -> the pieces'
    outputs concatenated, as model_forward returns them."""
    ys, hs, t0 = [], [], 0
    for n in cuts:
        y, h, state = model_forward(np.asarray(x)[:, t0:t0 + n], weights, K, mask_value, recurrent_activation, state)
        ys.append(y)
        hs.append(h)
        t0 += n
    assert t0 == np.asarray(x).shape[1]
    return np.concatenate(ys, axis=1), np.concatenate(hs, axis=1), state


def loss_and_grads(x, y, w, weights, K, mask_value=-1.0, recurrent_activation="hard_sigmoid", state=None):
    """lstm_train_ref.loss_and_grads with a detached entering state: (sum over frames of w * mean_F (xm s - y)^2,
    #frames with w != 0, [gradient of every weight array, Keras order], (final_h, final_c)) -- unnormalised sums;
    no gradient flows into (or is returned for) the entering state."""
    x = _t64(x)
    ws = [torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for v in weights]
    ks, rs, bs = ws[0:3 * K:3], ws[1:3 * K:3], ws[2:3 * K:3]
    ih, ic = state if state is not None else (None, None)
    hs, fh, fc = lstm_layers(x, ks, rs, bs, mask_value, recurrent_activation, ih, ic)
    s = R.head(hs[-1], ws[3 * K], ws[3 * K + 1])
    xm = x * R.valid_frames(x, mask_value).unsqueeze(-1)
    w, y = _t64(w), _t64(y)
    loss = (w * ((xm * s - y) ** 2).mean(dim=-1)).sum()
    loss.backward()
    return (float(loss.detach()), float((w != 0).sum()), [v.grad.numpy() for v in ws],
            (fh.detach().numpy(), fc.detach().numpy()))


def random_state(rng, K, B, H, scale=1.0):
    """(h, c) float32 [K,B,H] of magnitude about `scale`: h inside (-1, 1) as an LSTM output is."""
    h = np.tanh(scale * rng.standard_normal((K, B, H))).astype(np.float32)
    c = (scale * rng.standard_normal((K, B, H))).astype(np.float32)
    return h, c
