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
