"""fp64 reference of the LSTM baseline's training loss and gradients (enhance.py:1260-1312), built on the forward
restatement in tests/lstm_ref.py.  Differentiable with torch autograd; no GPU needed."""
import numpy as np
import torch

import lstm_ref as R


def loss_and_grads(x, y, w, weights, K, mask_value=-1.0, recurrent_activation="hard_sigmoid"):
    """The training loss 'mse_of_masked' with temporal sample weights, fp64 autograd: per frame
    w * mean_F (xm * s - y)^2 with xm = the Masking layer's output (masked frames zero) and s the sigmoid output.
    Returns (sum over frames, #frames with w != 0, [gradient of every weight array, Keras order]) -- the
    UNNORMALISED sums the kernels produce."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float64))
    ws = [torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for v in weights]
    ks, rs, bs = ws[0:3 * K:3], ws[1:3 * K:3], ws[2:3 * K:3]
    hs = R.lstm_layers(x, ks, rs, bs, mask_value, recurrent_activation)
    s = R.head(hs[-1], ws[3 * K], ws[3 * K + 1])
    xm = x * R.valid_frames(x, mask_value).unsqueeze(-1)
    w = torch.as_tensor(np.asarray(w, dtype=np.float64))
    y = torch.as_tensor(np.asarray(y, dtype=np.float64))
    per = ((xm * s - y) ** 2).mean(dim=-1)
    loss = (w * per).sum()
    loss.backward()
    return float(loss.detach()), float((w != 0).sum()), [v.grad.numpy() for v in ws]


# ---- the stages one at a time (tests/test_gpu_lstm_train_edges.py) ------------------------------------------------

def _t64(v):
    return v.detach().double() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, dtype=np.float64))


def head_loss_and_grads(xm, hidden, y, w, w_out, b_out):
    """The loss head alone, the contract of drnmf_lstm_loss_head_backward for ANY hidden [B,T,H]: per frame
    w * mean_F (xm * sigmoid(hidden @ w_out + b_out) - y)^2 with xm the Masking layer's output.  Returns (sum over
    frames, #frames with w != 0, d_hidden, d_w_out, d_b_out) -- unnormalised fp64 autograd gradients."""
    hidden, w_out, b_out = (_t64(v).clone().requires_grad_(True) for v in (hidden, w_out, b_out))
    xm, y, w = _t64(xm), _t64(y), _t64(w)
    s = R.head(hidden, w_out, b_out)
    loss = (w * ((xm * s - y) ** 2).mean(dim=-1)).sum()
    loss.backward()
    return (float(loss.detach()), float((w != 0).sum()), hidden.grad.numpy(), w_out.grad.numpy(),
            b_out.grad.numpy())


def hidden_vjp(x, weights, K, cot, mask_value=-1.0, recurrent_activation="hard_sigmoid", state=None):
    """The BPTT alone, the contract of drnmf_lstm_backward for ANY d_hidden: the vector-Jacobian product
    torch.autograd.grad(last layer's outputs [B,T,H], lstm weights, grad_outputs=cot), Keras order (3 K arrays:
    kernel, recurrent_kernel, bias per layer).  weights: the Keras list (arrays behind the first 3 K are ignored);
    state = (h, c) [K,B,H], a constant entering state as in tests/lstm_state_ref.py, or None."""
    import lstm_state_ref as SR
    ws = [torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for v in weights[:3 * K]]
    ih, ic = state if state is not None else (None, None)
    hs, _, _ = SR.lstm_layers(_t64(x), ws[0::3], ws[1::3], ws[2::3], mask_value, recurrent_activation, ih, ic)
    if not hs[-1].requires_grad:                      # (no valid frame at all: nothing depends on the weights)
        return [np.zeros(tuple(v.shape)) for v in ws]
    gs = torch.autograd.grad(hs[-1], ws, grad_outputs=_t64(cot), allow_unused=True)
    return [np.zeros(tuple(v.shape)) if g is None else g.numpy() for v, g in zip(ws, gs)]


def kink_margin(x, weights, K, mask_value=-1.0, state=None):
    """How far the fp64 run stays from the kinks of hard_sigmoid: the smallest distance, over valid frames, layers
    and the i, f, o gates, of 0.2 z + 0.5 from 0 and from 1 (inf without a valid frame).  A gate closer to a kink
    than the fp32 rounding of z may take the other branch on the device, where its derivative differs by 0.2: a
    test with a max-based bound asserts this margin first.  It depends on the reference alone."""
    import lstm_state_ref as SR
    x = _t64(x)
    m = R.valid_frames(x, mask_value)
    ws = [_t64(v) for v in weights[:3 * K]]
    ih, ic = state if state is not None else (None, None)
    hs, _, _ = SR.lstm_layers(x, ws[0::3], ws[1::3], ws[2::3], mask_value, "hard_sigmoid", ih, ic)
    inp = x * m.unsqueeze(-1)
    best = float("inf")
    for k in range(K):
        W, U, b = ws[3 * k], ws[3 * k + 1], ws[3 * k + 2]
        H = U.shape[0]
        h0 = torch.zeros(x.shape[0], 1, H, dtype=torch.float64) if ih is None else _t64(ih)[k].unsqueeze(1)
        prev = torch.cat([h0, hs[k][:, :-1]], dim=1)             # h_{t-1} of every frame
        z = inp @ W + prev @ U + b
        p = 0.2 * torch.cat([z[..., :2 * H], z[..., 3 * H:]], dim=-1) + 0.5
        p = p[m]
        if p.numel():
            best = min(best, float(torch.minimum(p.abs(), (p - 1.0).abs()).min()))
        inp = hs[k]
    return best
