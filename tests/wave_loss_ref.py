"""fp64 references of the waveform criteria (include/drnmf_waveloss.h) and what their two test files share
(test_wave_loss_host.py on the CPU, test_gpu_wave_loss.py on the MI355X): the transpose of the masked inverse STFT
from its closed form, both losses with their gradients, the two mask heads' backward passes for a given cotangent
by autograd, and the table of cases.  numpy, torch on the CPU and the oracle only: no GPU needed.

The identity (checked by test_wave_loss_host.py against O.reconstruct to 1e-12): with s^ = reconstruct(m re, m im)
and g a cotangent of s^, G = the windowed transform of g on the forward frame grid (output sample s at padded
position s + N, frames 0 .. nf-1, conjugated as O.stft_mc conjugates),
    d_mask[t, f] = (c_f / N) (2 hop / N) (re[t, f] Re G[t, f] + im[t, f] Im G[t, f]),  c_0 = c_{N/2} = 1, else 2."""
import functools

import numpy as np
import torch

from oracle import drnmf_oracle as O
from oracle import drnmf_torch_ref as TR
import lstm_ref as LR

EPS = 1e-8                      # of the SI-SDR
KINDS = ("wave_mse", "si_sdr")

# (N, hop) of the transposed inverse: the fast sizes' wave body at a hop that divides N and one that does not, the
# general body at an odd and an even log2 N
VJP_SIZES = [(512, 128), (128, 64), (512, 160), (64, 16)]
# lengths of wave_loss: one block of 4096 samples short by one, one over it, and the smallest rows
LOSS_LENGTHS = [1, 2, 4095, 4097]
# rows below and at the head's GEMM threshold (csrc/head.hip HEAD_GEMM_MIN_ROWS = 2048)
HEAD_ROWS = [17 * 9, 2048]
HEAD_SHAPES = [(3, 33), (100, 33), (3, 257), (100, 257)]          # (r, F)
LSTM_HEAD_SHAPES = [(3, 2, 9, 13), (17, 9, 33, 54), (5, 7, 33, 70)]        # (B, T, F, H)
G_TOL = 2e-3                    # tests/test_gpu_train.py, tests/test_gpu_lstm_train.py: max|d| / max|ref| per array
TOL_FWD = 2e-5                  # tests/stft_hops_ref.py: the forward transform's bound, of the row's largest value


def vjp_lengths(N, hop):
    return [1, hop - 1, hop + 1, 3 * hop + 7]


def frames(n, N, hop):
    return -(-n // hop) + N // hop + 1


def out_length(n, N, hop, crop=False):
    full = max(hop * (frames(n, N, hop) - 1) - N, 0)
    return min(full, n) if crop else full


def vjp(re, im, g, N, hop, n_out):
    """d_mask [nf, F] fp64 of the formula above: re, im [nf, F] in the stored (conjugated) convention, g the
    cotangent of the reconstruction, of which the first n_out samples count."""
    re, im = np.asarray(re, np.float64), np.asarray(im, np.float64)
    nf, F = re.shape
    assert F == N // 2 + 1
    gp = np.zeros(N + hop * (nf - 1) + N, np.float64)
    gp[N:N + n_out] = np.asarray(g, np.float64)[:n_out]
    w = O.sqrt_hann(N).astype(np.float64)
    idx = np.arange(N)[None, :] + hop * np.arange(nf)[:, None]
    G = np.conj(np.fft.fft(w[None, :] * gp[idx], axis=1)[:, :F])
    c = np.full(F, 2.0)
    c[0] = c[-1] = 1.0
    return (c / N) * (2.0 * hop / N) * (re * G.real + im * G.imag)


def wave_loss(est, ref, kind):
    """(loss, counted, g) of one row in fp64, g = d loss / d est in closed form; an empty row, and under 'si_sdr' a
    row whose reference is all zero, is not counted: loss 0, g 0."""
    a, s = np.asarray(est, np.float64), np.asarray(ref, np.float64)
    n = a.shape[0]
    assert kind in KINDS
    if n == 0:
        return 0.0, False, np.zeros(0)
    if kind == "wave_mse":
        return float(np.mean((a - s) ** 2)), True, 2.0 / n * (a - s)
    p, q, e = float(a @ s), float(s @ s), float(a @ a)
    if q == 0.0:
        return 0.0, False, np.zeros(n)
    c = 10.0 / np.log(10.0)
    t = p * p / q
    r = e - t
    loss = -c * (np.log(t + EPS) - np.log(r + EPS))
    g = 2.0 * c / (r + EPS) * a - (2.0 * p / q) * c * (1.0 / (t + EPS) + 1.0 / (r + EPS)) * s
    return float(loss), True, g


def wave_loss_torch(est, ref, kind):
    """The loss definition as a differentiable fp64 torch expression (est, ref tensors of one counted row)."""
    if kind == "wave_mse":
        return ((est - ref) ** 2).mean()
    p, q, e = (est * ref).sum(), (ref * ref).sum(), (est * est).sum()
    t = p * p / q
    return -10.0 * torch.log10((t + EPS) / (e - t + EPS))


def _t(v):
    return v.detach().cpu().double() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, np.float64))


def head_cot_grads(hidden, kc, kn, d_mask, square=False):
    """The ratio-mask head's backward for a given cotangent, by fp64 autograd of sum(mask * d_mask): hidden
    [rows, 2r], kc, kn [r, F], d_mask [rows, F] -> (d_hidden, d_kc, d_kn)."""
    hidden, kc, kn = (_t(v).clone().requires_grad_(True) for v in (hidden, kc, kn))
    z = torch.zeros(tuple(hidden.shape[:-1]) + (kc.shape[1],), dtype=torch.float64)
    _, _, mask = TR.head_terms(z, z, torch.ones(tuple(hidden.shape[:-1]), dtype=torch.float64), hidden, kc, kn, square)
    (mask * _t(d_mask)).sum().backward()
    return hidden.grad.numpy(), kc.grad.numpy(), kn.grad.numpy()


def lstm_head_cot_grads(hidden, w_out, b_out, d_mask):
    """The sigmoid head's backward for a given cotangent: hidden [B,T,H], w_out [H,F], b_out [F], d_mask [B,T,F]
    -> (d_hidden, d_w_out, d_b_out), fp64 autograd of sum(sigmoid(hidden w_out + b_out) * d_mask)."""
    hidden, w_out, b_out = (_t(v).clone().requires_grad_(True) for v in (hidden, w_out, b_out))
    (LR.head(hidden, w_out, b_out) * _t(d_mask)).sum().backward()
    return hidden.grad.numpy(), w_out.grad.numpy(), b_out.grad.numpy()


def reconstruct_torch(re, im, mask, N, hop, n_out):
    """O.reconstruct as a differentiable fp64 torch expression: re, im [nf, F] constants (stored convention), mask
    [nf, F] a tensor; the first n_out samples of the trimmed overlap-add."""
    re, im = _t(re), _t(im)
    nf, F = re.shape
    w = torch.as_tensor(O.sqrt_hann(N).astype(np.float64)) * (2.0 / (N / hop))
    S = torch.complex(mask * re, -(mask * im))                   # un-conjugated half spectrum
    S = torch.cat([torch.complex(S.real[:, :1], torch.zeros(nf, 1, dtype=torch.float64)), S[:, 1:-1],
                   torch.complex(S.real[:, -1:], torch.zeros(nf, 1, dtype=torch.float64))], dim=1)
    fr = torch.fft.irfft(S, n=N, dim=1) * w[None, :]
    y = torch.zeros(N + hop * (nf - 1), dtype=torch.float64)
    for i in range(nf):
        y = y + torch.nn.functional.pad(fr[i], (i * hop, hop * (nf - 1 - i)))
    return y[N:N + n_out]


def rel_err(got, ref):
    d, scale = float(np.max(np.abs(got - ref))) if ref.size else 0.0, float(np.max(np.abs(ref))) if ref.size else 0.0
    if scale == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / scale


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def vjp_case(N, hop, int16):
    """One ragged batch of a size, computed once and never modified: (lens, pcm [n, stride] with junk behind every
    length, masks per row [nf, F] float32, cotangents g [n, width] float32 with junk behind every output length)."""
    lens = vjp_lengths(N, hop)
    rng = np.random.default_rng(11 * N + hop + int(int16))
    stride = max(lens) + 3
    if int16:
        pcm = rng.integers(-20000, 20000, size=(len(lens), stride)).astype(np.int16)
    else:
        pcm = (0.3 * rng.standard_normal((len(lens), stride))).astype(np.float32)
    masks = tuple(_frozen(rng.random((frames(n, N, hop), N // 2 + 1)).astype(np.float32)) for n in lens)
    width = max(out_length(n, N, hop) for n in lens) + 5
    g = _frozen(rng.standard_normal((len(lens), width)).astype(np.float32))
    return lens, _frozen(pcm), masks, g
