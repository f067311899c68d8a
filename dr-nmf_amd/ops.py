"""Torch-tensor front end of the C ABI: tensors are device-memory containers only; every op
enqueues hand-written HIP kernels on torch's current stream through libdrnmf.so."""
import ctypes as C

import numpy as np

import torch

from . import _capi

ACTIVATIONS = _capi.ACTIVATIONS


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev_index(t):
    if not t.is_cuda:
        raise ValueError("drnmf_amd ops need CUDA(HIP) tensors; got a %s tensor. There is no CPU "
                         "fallback." % t.device)
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def _dev_of(d):
    """Device index of an int, a torch.device / device string, or a CUDA tensor."""
    if isinstance(d, int):
        return d
    if isinstance(d, torch.Tensor):
        return _dev_index(d)
    d = torch.device(d)
    if d.type != 'cuda':
        raise ValueError("drnmf_amd ops need a CUDA(HIP) device; got %s. There is no CPU fallback." % d)
    return d.index if d.index is not None else torch.cuda.current_device()


def _f32c(t, name):
    if t.dtype != torch.float32:
        raise ValueError("%s must be float32 (got %s)" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


# ---- the argument rules every wrapper below shares: one call sequence, one output check, one workspace rule ----
def _call(name, dev, *args, stream=True):
    """The C entry `name` on device index `dev`'s handle: name(handle, *args[, torch's current stream]), then
    _capi.check.  Arguments are passed as they are (the site converts them, in the header's order)."""
    L = _capi.lib()
    h = _capi.handle(dev)
    rc = getattr(L, name)(h, *args, _stream()) if stream else getattr(L, name)(h, *args)
    _capi.check(rc, h, name)


def _given(t, shape, dtype, device, name):
    """The one test of a tensor the caller supplies for a kernel to write: contiguous, `dtype`, exactly `shape`
    (a tuple), on `device` (a tensor's .device) -- ValueError otherwise.  Returns t."""
    if tuple(t.shape) != shape or t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s tensor of shape %s on %s (got %s %s on %s)" %
                         (name, dtype, shape, device, t.dtype, tuple(t.shape), t.device))
    return t


def _out(out, shape, dtype, device, name="out"):
    """Allocate or check: a new tensor when `out` is None, else `out` itself if it passes `_given`."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    return _given(out, shape, dtype, device, name)


def _check_state(t, shape, device, name):
    """A float32 state the caller may leave out: None passes, anything else must pass `_given`."""
    if t is not None:
        _given(t, shape, torch.float32, device, name)


def _workspace(need, device, have=None):
    """`have` itself when it is a uint8 tensor of at least `need` bytes on `device`, else a new one."""
    if have is not None and have.dtype == torch.uint8 and have.numel() >= need and \
            have.device == torch.device(device):
        return have
    return torch.empty(max(need, 1), dtype=torch.uint8, device=device)


def _mask_pair(mask_value):
    """(value, given) as the SNMF family's entries take a mask value."""
    return (0.0, 0) if mask_value is None else (float(mask_value), 1)


def _mask_nan(mask_value):
    """The cell family's convention: NaN means no masking."""
    return float("nan") if mask_value is None else float(mask_value)


def _hidden_width(desc):
    """Last dimension of a cell's output: every layer's state with return_all_hidden, else the last one's."""
    return desc.N * (desc.K if desc.return_all_hidden else 1)


DIVERGENCES ={"ed": _capi.DIV_ED, "kl": _capi.DIV_KL, "beta": _capi.DIV_BETA}


def make_desc(B, T, F, N, K, n_D=1, n_alph=1, alph_len=1, n_lam=1, return_all_hidden=False,
              operand_f16=False, divergence="ed"):
    if divergence not in DIVERGENCES:
        raise ValueError("divergence must be 'ed', 'kl' or 'beta'")
    return _capi.CellDesc(int(B), int(T), int(F), int(N), int(K), int(n_D), int(n_alph),
                          int(alph_len), int(n_lam), int(bool(return_all_hidden)),
                          int(bool(operand_f16)), DIVERGENCES[divergence])


def prepare_params(desc, log_D, log_alph, log_lam1, out=None):
    """log_D [n_D,F,N], log_alph [n_alph,alph_len], log_lam1 [n_lam] -> prepared block (uint8)."""
    dev = _dev_index(log_D)
    log_D, log_alph, log_lam1 = (_f32c(log_D, "log_D"), _f32c(log_alph, "log_alph"),
                                 _f32c(log_lam1, "log_lam1"))
    if log_D.numel() != desc.n_D * desc.F * desc.N:
        raise ValueError("log_D has %d elements, expected n_D*F*N = %d" %
                         (log_D.numel(), desc.n_D * desc.F * desc.N))
    if log_alph.numel() != desc.n_alph * desc.alph_len or log_lam1.numel() != desc.n_lam:
        raise ValueError("log_alph/log_lam1 sizes do not match the descriptor")
    out = _workspace(_capi.lib().drnmf_params_bytes(C.byref(desc)), log_D.device, out)
    _call("drnmf_prepare_params", dev, C.byref(desc), _capi.ptr(log_D), _capi.ptr(log_alph),
          _capi.ptr(log_lam1), _capi.ptr(out))
    return out


def unpack_params(block, desc):
    """Unpacked copies/views of a prepared block: (Dn [n_D,Fp,Np], colnorm [n_D,Np], inv_alpha [K,Np],
    bias [K,Np]) -- the layout of params_layout() in csrc/common.h."""
    Fp = (desc.F + 15) // 16 * 16
    Np = (desc.N + 31) // 32 * 32
    r256 = lambda v: (v + 255) // 256 * 256
    f = block.view(torch.float32) if block.dtype != torch.float32 else block
    o = 0
    n = desc.n_D * Fp * Np
    # tile-packed Dp[ft][ac][q][f%16][e] (n%16 = 4q + e) -> logical [Fp][Np]
    Dn = f[o:o + n].view(desc.n_D, Fp // 16, Np // 16, 4, 16, 4).permute(0, 1, 4, 2, 3, 5) \
        .reshape(desc.n_D, Fp, Np); o += n
    n = desc.n_D * Np
    colnorm = f[o:o + n].view(desc.n_D, Np); o += r256(n * 4) // 4
    n = desc.K * Np
    inv_alpha = f[o:o + n].view(desc.K, Np); o += r256(n * 4) // 4
    bias = f[o:o + n].view(desc.K, Np)
    return Dn, colnorm, inv_alpha, bias


def cell_launches_per_frame(desc):
    """Chain launches per frame of the forward for this descriptor (2K-1 factored, K-1 Gram form)."""
    return int(_capi.lib().drnmf_cell_launches_per_frame(C.byref(desc)))


def cell_workspace(desc, device):
    nbytes = _capi.lib().drnmf_cell_workspace_bytes(C.byref(desc))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def cell_forward(x, mask_value, params, desc, log_h0, u, out=None, workspace=None,
                 initial_state=None, final_state=None):
    """x [B,T,F] -> h [B,T,N] (or [B,T,K*N]).  mask_value None = no masking.
    u = (u0_diag, u0_off, uk_off).  initial_state / final_state [B,N]: stateful mode."""
    dev = _dev_index(x)
    x = _f32c(x, "x")
    log_h0 = _f32c(log_h0, "log_h0")
    if tuple(x.shape) != (desc.B, desc.T, desc.F):
        raise ValueError("x has shape %s, descriptor says (%d,%d,%d)" %
                         (tuple(x.shape), desc.B, desc.T, desc.F))
    if log_h0.numel() != desc.N:
        raise ValueError("log_h0 must have N=%d elements" % desc.N)
    out = _out(out, (desc.B, desc.T, _hidden_width(desc)), torch.float32, x.device)
    if workspace is None:
        workspace = cell_workspace(desc, x.device)
    mv = _mask_nan(mask_value)
    if initial_state is not None or final_state is not None:
        _check_state(initial_state, (desc.B, desc.N), x.device, "initial_state")
        _check_state(final_state, (desc.B, desc.N), x.device, "final_state")
        _call("drnmf_cell_forward_stateful", dev, C.byref(desc), _capi.ptr(x), mv, _capi.ptr(params),
              _capi.ptr(log_h0), float(u[0]), float(u[1]), float(u[2]), _capi.ptr(initial_state),
              _capi.ptr(final_state), _capi.ptr(out), _capi.ptr(workspace), workspace.numel())
        return out
    _call("drnmf_cell_forward", dev, C.byref(desc), _capi.ptr(x), mv, _capi.ptr(params), _capi.ptr(log_h0),
          float(u[0]), float(u[1]), float(u[2]), _capi.ptr(out), _capi.ptr(workspace), workspace.numel())
    return out


def make_dense_desc(B, T, F, N, K, connect_input=True, activation="relu",
                    return_all_hidden=False, operand_f16=False):
    if activation not in _capi.ACTIVATIONS:
        raise ValueError("activation %r is not one of %s" % (activation,
                                                             sorted(_capi.ACTIVATIONS)))
    return _capi.DenseDesc(int(B), int(T), int(F), int(N), int(K), int(bool(connect_input)),
                           _capi.ACTIVATIONS[activation], int(bool(return_all_hidden)),
                           int(bool(operand_f16)))


def dense_prepare_params(desc, U, S, W, b, out=None):
    """U [K,N,N], S [K-1,N,N] (None when K == 1), W [K,F,N] (None without the input connection),
    b [K,N] -- the reference's Uk/Sk/Wk/bk lists stacked -> prepared block (uint8)."""
    dev = _dev_index(U)
    K, N, F = desc.K, desc.N, desc.F
    U, b = _f32c(U, "U"), _f32c(b, "b")
    if tuple(U.shape) != (K, N, N) or tuple(b.shape) != (K, N):
        raise ValueError("U/b must have shapes (K,N,N)/(K,N) = (%d,%d,%d)/(%d,%d)" % (K, N, N, K, N))
    if K > 1:
        S = _f32c(S, "S")
        if tuple(S.shape) != (K - 1, N, N):
            raise ValueError("S must have shape (K-1,N,N)")
    else:
        S = None
    if desc.connect_input:
        W = _f32c(W, "W")
        if tuple(W.shape) != (K, F, N):
            raise ValueError("W must have shape (K,F,N) = (%d,%d,%d)" % (K, F, N))
    else:
        W = None
    out = _workspace(_capi.lib().drnmf_dense_params_bytes(C.byref(desc)), U.device, out)
    _call("drnmf_dense_prepare_params", dev, C.byref(desc), _capi.ptr(U), _capi.ptr(S), _capi.ptr(W),
          _capi.ptr(b), _capi.ptr(out))
    return out


def dense_workspace(desc, device):
    nbytes = _capi.lib().drnmf_dense_workspace_bytes(C.byref(desc))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _check_drop_u(drop_u, desc):
    drop_u = _f32c(drop_u, "drop_u")
    if tuple(drop_u.shape) != (desc.B, desc.N):
        raise ValueError("drop_u must be a (B,N) = (%d,%d) mask" % (desc.B, desc.N))
    return drop_u


def dense_cell_forward(x, mask_value, params, desc, h0, out=None, workspace=None,
                       initial_state=None, final_state=None, drop_u=None):
    """General SimpleDeepRNN.step on dense per-layer matrices: x [B,T,F] -> h [B,T,N] (or
    [B,T,K*N]).  h0 [N] is the initial state itself.  drop_u [B,N]: the training phase's recurrent
    dropout mask B_U (custom_layers.py:377-384), 0 or 1/(1-p)."""
    dev = _dev_index(x)
    x, h0 = _f32c(x, "x"), _f32c(h0, "h0")
    if tuple(x.shape) != (desc.B, desc.T, desc.F):
        raise ValueError("x has shape %s, descriptor says (%d,%d,%d)" %
                         (tuple(x.shape), desc.B, desc.T, desc.F))
    if h0.numel() != desc.N:
        raise ValueError("h0 must have N=%d elements" % desc.N)
    out = _out(out, (desc.B, desc.T, _hidden_width(desc)), torch.float32, x.device)
    if workspace is None:
        workspace = dense_workspace(desc, x.device)
    _check_state(initial_state, (desc.B, desc.N), x.device, "initial_state")
    _check_state(final_state, (desc.B, desc.N), x.device, "final_state")
    mv = _mask_nan(mask_value)
    if drop_u is not None and (initial_state is not None or final_state is not None):
        # a stateful layer in its training phase (custom_layers.py:296-318 with 377-384)
        drop_u = _check_drop_u(drop_u, desc)
        _call("drnmf_dense_cell_forward_dropout_stateful", dev, C.byref(desc), _capi.ptr(x), mv, _capi.ptr(params),
              _capi.ptr(h0), _capi.ptr(initial_state), _capi.ptr(final_state), _capi.ptr(drop_u), _capi.ptr(out),
              _capi.ptr(workspace), workspace.numel())
        return out
    if drop_u is not None:
        drop_u = _check_drop_u(drop_u, desc)
        _call("drnmf_dense_cell_forward_dropout", dev, C.byref(desc), _capi.ptr(x), mv, _capi.ptr(params),
              _capi.ptr(h0), _capi.ptr(drop_u), _capi.ptr(out), _capi.ptr(workspace), workspace.numel())
        return out
    _call("drnmf_dense_cell_forward", dev, C.byref(desc), _capi.ptr(x), mv, _capi.ptr(params), _capi.ptr(h0),
          _capi.ptr(initial_state), _capi.ptr(final_state), _capi.ptr(out), _capi.ptr(workspace),
          workspace.numel())
    return out


def dense_cell_backward(x, mask_value, desc, U, S, W, b, h0, hall, d_out, workspace=None,
                        drop_u=None, initial_state=None):
    """BPTT of the dense step (drnmf_dense_cell_backward): hall [B,T,K*N] is the forward's
    all-hidden output, d_out the gradient w.r.t. the returned output ([B,T,N], or [B,T,K*N] when
    desc.return_all_hidden).  Returns dict(dU [K,N,N], dS [K-1,N,N] | None, dW [K,F,N] | None,
    db [K,N], dh0 [N]).  initial_state [B,N]: the state a stateful layer's batch entered with
    (drnmf_dense_cell_backward_stateful: a constant of the gradient, dh0 = 0)."""
    di = _dev_index(x)
    B, T, F, N, K = desc.B, desc.T, desc.F, desc.N, desc.K
    x, U, b, h0 = _f32c(x, "x"), _f32c(U, "U"), _f32c(b, "b"), _f32c(h0, "h0")
    hall, d_out = _f32c(hall, "hall"), _f32c(d_out, "d_out")
    width = _hidden_width(desc)
    if tuple(x.shape) != (B, T, F) or tuple(hall.shape) != (B, T, K * N) or \
            tuple(d_out.shape) != (B, T, width):
        raise ValueError("x / hall / d_out must have shapes (B,T,F) / (B,T,K*N) / (B,T,%d)" % width)
    if tuple(U.shape) != (K, N, N) or tuple(b.shape) != (K, N) or h0.numel() != N:
        raise ValueError("U / b / h0 must have shapes (K,N,N) / (K,N) / (N,)")
    dev = x.device
    S = _f32c(S, "S") if K > 1 else None
    W = _f32c(W, "W") if desc.connect_input else None
    g = dict(dU=torch.empty((K, N, N), dtype=torch.float32, device=dev),
             dS=torch.empty((K - 1, N, N), dtype=torch.float32, device=dev) if K > 1 else None,
             dW=torch.empty((K, F, N), dtype=torch.float32, device=dev) if desc.connect_input
             else None,
             db=torch.empty((K, N), dtype=torch.float32, device=dev),
             dh0=torch.empty((N,), dtype=torch.float32, device=dev))
    g["workspace"] = workspace = _workspace(_capi.lib().drnmf_dense_backward_workspace_bytes(C.byref(desc)), dev,
                                            workspace)
    mv = _mask_nan(mask_value)
    head = (C.byref(desc), _capi.ptr(x), mv, _capi.ptr(U), _capi.ptr(S), _capi.ptr(W), _capi.ptr(b))
    if initial_state is not None:
        _check_state(initial_state, (B, N), dev, "initial_state")
        if drop_u is not None:
            drop_u = _check_drop_u(drop_u, desc)
        _call("drnmf_dense_cell_backward_stateful", di, *head, _capi.ptr(initial_state), _capi.ptr(drop_u),
              _capi.ptr(hall), _capi.ptr(d_out), _capi.ptr(g["dU"]), _capi.ptr(g["dS"]), _capi.ptr(g["dW"]),
              _capi.ptr(g["db"]), _capi.ptr(workspace), workspace.numel())
        g["dh0"].zero_()
        return g
    if drop_u is not None:
        drop_u = _check_drop_u(drop_u, desc)
        _call("drnmf_dense_cell_backward_dropout", di, *head, _capi.ptr(h0), _capi.ptr(drop_u), _capi.ptr(hall),
              _capi.ptr(d_out), _capi.ptr(g["dU"]), _capi.ptr(g["dS"]), _capi.ptr(g["dW"]), _capi.ptr(g["db"]),
              _capi.ptr(g["dh0"]), _capi.ptr(workspace), workspace.numel())
        return g
    _call("drnmf_dense_cell_backward", di, *head, _capi.ptr(h0), _capi.ptr(hall), _capi.ptr(d_out),
          _capi.ptr(g["dU"]), _capi.ptr(g["dS"]), _capi.ptr(g["dW"]), _capi.ptr(g["db"]), _capi.ptr(g["dh0"]),
          _capi.ptr(workspace), workspace.numel())
    return g


def cell_forward_ista(x, mask_value, params, desc, log_h0, beta=1.5, out=None, workspace=None,
                      initial_state=None, final_state=None):
    """KL / beta variant of the cell (desc.divergence = 'kl' | 'beta'): every frame runs K full
    ISTA steps of the reference's ista_kl / ista_beta warm-started from the previous frame's
    output.  x [B,T,F] -> h [B,T,N] (or [B,T,K*N])."""
    dev = _dev_index(x)
    x, log_h0 = _f32c(x, "x"), _f32c(log_h0, "log_h0")
    if tuple(x.shape) != (desc.B, desc.T, desc.F):
        raise ValueError("x has shape %s, descriptor says (%d,%d,%d)" %
                         (tuple(x.shape), desc.B, desc.T, desc.F))
    if log_h0.numel() != desc.N:
        raise ValueError("log_h0 must have N=%d elements" % desc.N)
    out = _out(out, (desc.B, desc.T, _hidden_width(desc)), torch.float32, x.device)
    if workspace is None:
        workspace = cell_workspace(desc, x.device)
    _check_state(initial_state, (desc.B, desc.N), x.device, "initial_state")
    _check_state(final_state, (desc.B, desc.N), x.device, "final_state")
    _call("drnmf_cell_forward_ista", dev, C.byref(desc), _capi.ptr(x), _mask_nan(mask_value), _capi.ptr(params),
          _capi.ptr(log_h0), float(beta), _capi.ptr(initial_state), _capi.ptr(final_state), _capi.ptr(out),
          _capi.ptr(workspace), workspace.numel())
    return out


def cell_profile(x, mask_value, params, desc, log_h0, u, out, workspace, frames=8):
    """Measurement aid: per-kernel mean durations (us) of the first `frames` frames, HIP events on
    the launch stream.  Returns dict(cell_a_us, cell_b_us, frame_us)."""
    res = (C.c_float * 3)()
    # (the stream is not this entry's last argument)
    _call("drnmf_cell_profile", _dev_index(x), C.byref(desc), _capi.ptr(x), _mask_nan(mask_value), _capi.ptr(params),
          _capi.ptr(log_h0), float(u[0]), float(u[1]), float(u[2]), _capi.ptr(out), _capi.ptr(workspace),
          workspace.numel(), _stream(), int(frames), res, stream=False)
    return {"cell_a_us": float(res[0]), "cell_b_us": float(res[1]), "frame_us": float(res[2])}


def head_forward(hidden, kernel_clean, kernel_noise, square=False, want_ab=False, h_off=0,
                 out=None):
    """hidden [..., ld] (uses columns h_off .. h_off+2r) -> mask [..., F] (and A, Bn)."""
    dev = _dev_index(hidden)
    hidden = _f32c(hidden, "hidden")
    kc, kn = _f32c(kernel_clean, "kernel_clean"), _f32c(kernel_noise, "kernel_noise")
    r, F = kc.shape
    if tuple(kn.shape) != (r, F):
        raise ValueError("kernel_noise shape %s != kernel_clean shape %s" %
                         (tuple(kn.shape), (r, F)))
    ld = hidden.shape[-1]
    rows = hidden.numel() // ld
    shape = tuple(hidden.shape[:-1]) + (F,)
    mask = _out(out, shape, torch.float32, hidden.device)
    A = torch.empty(shape, dtype=torch.float32, device=hidden.device) if want_ab else None
    Bn = torch.empty(shape, dtype=torch.float32, device=hidden.device) if want_ab else None
    Fp = _capi.lib().drnmf_padded_f(F)
    ecat = torch.empty(2 * ((r + 15) // 16 * 16) * Fp, dtype=torch.float32, device=hidden.device)
    _call("drnmf_head_forward", dev, rows, F, r, _capi.ptr(hidden), ld, int(h_off), _capi.ptr(kc), _capi.ptr(kn),
          int(bool(square)), _capi.ptr(mask), _capi.ptr(A), _capi.ptr(Bn), _capi.ptr(ecat))
    return (mask, A, Bn) if want_ab else mask


def _head_grad_outputs(out, kc, kn, dev):
    """(sums[2], d_kernel_clean, d_kernel_noise): the caller's `out` triple (contiguous fp32 device
    tensors of those sizes, e.g. views of a flat gradient buffer) or fresh tensors."""
    sums, dkc, dkn = (None, None, None) if out is None else out
    return (_out(sums, (2,), torch.float32, dev, "sums"),
            _out(dkc, tuple(kc.shape), torch.float32, dev, "d_kernel_clean"),
            _out(dkn, tuple(kn.shape), torch.float32, dev, "d_kernel_noise"))


def loss_head_backward(x_raw, hidden, kernel_clean, kernel_noise, mask, A, Bn, y, w, square=False,
                       h_off=0, out=None):
    """Unnormalised loss + gradients of the mask head (see drnmf_loss_head_backward).
    Returns (sums[2] device tensor, d_hidden [..., 2r], d_kernel_clean, d_kernel_noise); `out` =
    (sums, d_kernel_clean, d_kernel_noise) to write into."""
    di = _dev_index(hidden)
    x_raw, hidden, mask, A, Bn, y = (_f32c(t, n) for t, n in
                                     ((x_raw, "x_raw"), (hidden, "hidden"), (mask, "mask"),
                                      (A, "A"), (Bn, "Bn"), (y, "y")))
    w = _f32c(w, "w")
    kc, kn = _f32c(kernel_clean, "kernel_clean"), _f32c(kernel_noise, "kernel_noise")
    r, F = kc.shape
    ld = hidden.shape[-1]
    rows = hidden.numel() // ld
    if x_raw.numel() != rows * F or w.numel() != rows:
        raise ValueError("loss_head_backward: shape mismatch")
    dev = hidden.device
    sums, dkc, dkn = _head_grad_outputs(out, kc, kn, dev)
    d_hidden = torch.empty(tuple(hidden.shape[:-1]) + (2 * r,), dtype=torch.float32, device=dev)
    nbytes = _capi.lib().drnmf_loss_head_workspace_bytes(rows, F, r)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _call("drnmf_loss_head_backward", di, rows, F, r, _capi.ptr(x_raw), _capi.ptr(hidden), ld, int(h_off),
          _capi.ptr(kc), _capi.ptr(kn), int(bool(square)), _capi.ptr(mask), _capi.ptr(A), _capi.ptr(Bn),
          _capi.ptr(y), _capi.ptr(w), _capi.ptr(sums), _capi.ptr(d_hidden), _capi.ptr(dkc), _capi.ptr(dkn),
          _capi.ptr(ws), nbytes)
    return sums, d_hidden, dkc, dkn


def snmf_cost_head_backward(x_raw, hidden, kernel_clean, kernel_noise, A, Bn, w, l1_weight,
                            h_off=0, out=None):
    """Unnormalised SNMF-cost pretraining loss + head gradients (drnmf_snmf_cost_head_backward):
    per frame 0.5*mean_f (A+Bn-x)^2 + l1_weight*mean_n |h|.  Same returns as loss_head_backward."""
    di = _dev_index(hidden)
    x_raw, hidden, A, Bn, w = (_f32c(t, n) for t, n in
                               ((x_raw, "x_raw"), (hidden, "hidden"), (A, "A"), (Bn, "Bn"),
                                (w, "w")))
    kc, kn = _f32c(kernel_clean, "kernel_clean"), _f32c(kernel_noise, "kernel_noise")
    r, F = kc.shape
    ld = hidden.shape[-1]
    rows = hidden.numel() // ld
    if x_raw.numel() != rows * F or w.numel() != rows or A.numel() != rows * F:
        raise ValueError("snmf_cost_head_backward: shape mismatch")
    dev = hidden.device
    sums, dkc, dkn = _head_grad_outputs(out, kc, kn, dev)
    d_hidden = torch.empty(tuple(hidden.shape[:-1]) + (2 * r,), dtype=torch.float32, device=dev)
    nbytes = _capi.lib().drnmf_loss_head_workspace_bytes(rows, F, r)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _call("drnmf_snmf_cost_head_backward", di, rows, F, r, _capi.ptr(x_raw), _capi.ptr(hidden), ld, int(h_off),
          _capi.ptr(kc), _capi.ptr(kn), _capi.ptr(A), _capi.ptr(Bn), _capi.ptr(w), float(l1_weight),
          _capi.ptr(sums), _capi.ptr(d_hidden), _capi.ptr(dkc), _capi.ptr(dkn), _capi.ptr(ws), nbytes)
    return sums, d_hidden, dkc, dkn


def cell_backward(x, params, desc, log_h0, u, hall, d_out, fwd_workspace, grads=None, profile=None,
                  beta=None, initial_state=None):
    """BPTT through the cell (forward must have been run with return_all_hidden=True on the same
    workspace).  A KL / beta descriptor (desc.divergence) goes to drnmf_cell_backward_ista with
    `beta` (u is ignored: that cell has no U term).  Returns dict(d_log_D [n_D,F,N], d_log_alph [n_alph,alph_len], d_log_lam1 [n_lam],
    d_log_h0 [N]); `grads` may supply preallocated output tensors.  `profile` (a dict, bench.py
    only) switches to drnmf_cell_backward_profile, which synchronises and fills chain_ms /
    batched_ms / chain_launches.  initial_state [B,N]: stateful training -- the forward was
    cell_forward(..., initial_state=...), the supplied state is a constant of the gradient
    (drnmf_cell_backward_stateful; d_log_h0 comes back zero)."""
    di = _dev_index(x)
    x, hall, d_out = _f32c(x, "x"), _f32c(hall, "hall"), _f32c(d_out, "d_out")
    if tuple(hall.shape) != (desc.B, desc.T, desc.K * desc.N):
        raise ValueError("hall must be (B,T,K*N) = (%d,%d,%d)" % (desc.B, desc.T, desc.K * desc.N))
    if tuple(d_out.shape) != (desc.B, desc.T, desc.N):
        raise ValueError("d_out must be (B,T,N)")
    dev = x.device
    g = grads or {}
    out = {
        "d_log_D": g.get("d_log_D", None) if g.get("d_log_D") is not None else
        torch.empty((desc.n_D, desc.F, desc.N), dtype=torch.float32, device=dev),
        "d_log_alph": g.get("d_log_alph") if g.get("d_log_alph") is not None else
        torch.empty((desc.n_alph, desc.alph_len), dtype=torch.float32, device=dev),
        "d_log_lam1": g.get("d_log_lam1") if g.get("d_log_lam1") is not None else
        torch.empty((desc.n_lam,), dtype=torch.float32, device=dev),
        "d_log_h0": g.get("d_log_h0") if g.get("d_log_h0") is not None else
        torch.empty((desc.N,), dtype=torch.float32, device=dev),
    }
    nbytes = _capi.lib().drnmf_cell_backward_workspace_bytes(C.byref(desc))
    bws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    # every entry: head, its step parameters (u, or beta for the KL / beta cell), [the entering state], tail
    head = (C.byref(desc), _capi.ptr(x), _capi.ptr(params), _capi.ptr(log_h0))
    step = (float(u[0]), float(u[1]), float(u[2]))
    tail = (_capi.ptr(hall), _capi.ptr(d_out), _capi.ptr(fwd_workspace), fwd_workspace.numel(), _capi.ptr(bws),
            nbytes, _capi.ptr(out["d_log_D"]), _capi.ptr(out["d_log_alph"]), _capi.ptr(out["d_log_lam1"]),
            _capi.ptr(out["d_log_h0"]))
    ista = desc.divergence != _capi.DIV_ED
    if ista:
        step = (float(1.5 if beta is None else beta),)
    if initial_state is not None:
        if profile is not None:
            raise NotImplementedError("stateful BPTT: unprofiled")
        _check_state(initial_state, (desc.B, desc.N), dev, "initial_state")
        _call("drnmf_cell_backward_ista_stateful" if ista else "drnmf_cell_backward_stateful", di, *head, *step,
              _capi.ptr(initial_state), *tail)
    elif ista:
        _call("drnmf_cell_backward_ista", di, *head, *step, *tail)
    elif profile is not None:
        res = (C.c_float * 3)()
        # (the stream is not this entry's last argument)
        _call("drnmf_cell_backward_profile", di, *head, *step, *tail, _stream(), res, stream=False)
        profile.update(chain_ms=float(res[0]), batched_ms=float(res[1]),
                       chain_launches=int(res[2]))
    else:
        _call("drnmf_cell_backward", di, *head, *step, *tail)
    return out


def adam_step(param, grad, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    dev = _dev_index(param)
    for t in (param, grad, m, v):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("adam_step needs contiguous float32 tensors")
    _call("drnmf_adam_step", dev, param.numel(), _capi.ptr(param), _capi.ptr(grad), _capi.ptr(m), _capi.ptr(v),
          float(lr_t), float(beta1), float(beta2), float(eps), float(grad_scale))


def sumsq(g):
    # 256 partials, summed on the host
    return float(sumsq_partials(g).cpu().numpy().astype(np.float64).sum())


def sumsq_partials(g, out=None):
    """256 partial sums of g^2 left ON THE DEVICE (the global-norm clip of adam_step_flat reads them)."""
    dev = _dev_index(g)
    out = _out(out, (256,), torch.float32, g.device)
    _call("drnmf_sumsq", dev, g.numel(), _capi.ptr(_f32c(g, "g")), _capi.ptr(out))
    return out


ADAM_BLOCK = 1024          # elements per drnmf_adam_block_t entry


def adam_block_table(items, device):
    """Device table of drnmf_adam_block_t {float* param; int64 flat_off; int32 count; int32 reserved}
    for drnmf_adam_step_flat: `items` = [(name, tensor)] in flat-buffer order; the tensors must stay
    where they are (same storage) for as long as the table is used.  Returns (table, n_blocks)."""
    rows = []
    off = 0
    for _, t in items:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("adam_block_table needs contiguous float32 tensors")
        n, base = int(t.numel()), int(t.data_ptr())
        for e in range(0, n, ADAM_BLOCK):
            rows.append((base + 4 * e, off + e, min(ADAM_BLOCK, n - e), 0))
        off += n
    arr = np.zeros(len(rows), dtype=np.dtype([('param', '<u8'), ('flat_off', '<i8'),
                                              ('count', '<i4'), ('reserved', '<i4')]))
    for i, r in enumerate(rows):
        arr[i] = r
    table = torch.from_numpy(arr.view(np.uint8).copy()).to(device)
    return table, len(rows)


def adam_step_flat(table, n_blocks, flat_grad, flat_m, flat_v, scalars4, lr_t, beta1=0.9, beta2=0.999,
                   eps=1e-8, clipnorm=0.0, keras204=False, reg_loss=0.0, sumsq256=None, report=None):
    """ONE launch for the whole optimiser step; scale, clip and the fault guard are evaluated on the
    device from `scalars4` = [sum w*mse, count, frames, fault] (see include/drnmf.h).  `report`: 4 floats
    of device-accessible memory (e.g. a pinned host tensor) that receive [loss, fault, scale, count]."""
    _call("drnmf_adam_step_flat", _dev_index(flat_grad), int(n_blocks), _capi.ptr(table), _capi.ptr(flat_grad),
          _capi.ptr(flat_m), _capi.ptr(flat_v), _capi.ptr(scalars4), _capi.ptr(sumsq256), float(lr_t), float(beta1),
          float(beta2), float(eps), float(clipnorm), 1 if keras204 else 0, float(reg_loss),
          report if isinstance(report, int) else _capi.ptr(report))


def adam_step_flat_counted(table, n_blocks, flat_grad, flat_m, flat_v, scalars4, lr, decay, step_in, step_out,
                           beta1=0.9, beta2=0.999, eps=1e-8, clipnorm=0.0, keras204=False, reg_loss=0.0,
                           sumsq256=None, report=None):
    """adam_step_flat with the step count on the device: `step_in` / `step_out` are two DIFFERENT one-element
    float32 device tensors (applied steps before / after this launch); lr_t is evaluated by the launch."""
    _call("drnmf_adam_step_flat_counted", _dev_index(flat_grad), int(n_blocks), _capi.ptr(table),
          _capi.ptr(flat_grad), _capi.ptr(flat_m), _capi.ptr(flat_v), _capi.ptr(scalars4), _capi.ptr(sumsq256),
          float(lr), float(decay), float(beta1), float(beta2), float(eps), float(clipnorm), 1 if keras204 else 0,
          float(reg_loss), _capi.ptr(step_in), _capi.ptr(step_out),
          report if isinstance(report, int) else _capi.ptr(report))


_report_rings = {}


def host_report_ring(device):
    """(numpy view [slots, 4] of the handle's host-mapped report ring, its base address) -- a slot's
    address is a valid `report` argument of adam_step_flat."""
    dev = _dev_of(device)
    if dev not in _report_rings:
        p = C.POINTER(C.c_float)()
        n = C.c_int32(0)
        _call("drnmf_host_report_ring", dev, C.byref(p), C.byref(n), stream=False)
        arr = np.ctypeslib.as_array(p, shape=(int(n.value), 4))
        _report_rings[dev] = (arr, C.addressof(p.contents))
    return _report_rings[dev]


def check_status(device):
    """Raise if an EARLIER, already synchronised call on this device's handle suffered an asynchronous
    fault (a persistent chain that timed out: its output is invalid).  Reads and clears the flag."""
    _call("drnmf_check_status", _dev_of(device), stream=False)


def persist_admitted(device):
    """True if this process's handle on `device` may run the persistent small-shape chains (it holds the
    device's cross-process lock; see include/drnmf.h)."""
    L = _capi.lib()
    return int(L.drnmf_persist_admitted(_capi.handle(_dev_of(device)))) == 1


def persist_admit_reason(device):
    """Why this process's handle on `device` is (not) admitted to the persistent chains (a sentence)."""
    L = _capi.lib()
    return L.drnmf_persist_admit_reason(_capi.handle(_dev_of(device))).decode()


def status_take(dst):
    """Stream-ordered: adds 1.0 to the one-element device tensor `dst` if the handle's fault word is
    raised, and clears it (no synchronisation)."""
    _call("drnmf_status_take_device", _dev_index(dst), _capi.ptr(dst))


def reload_env():
    """libdrnmf reads its DRNMF_* tuning variables once per process; call this after changing one."""
    _capi.lib().drnmf_reload_env()


MATRIX_MODES = {"f32": _capi.MATRIX_F32, "bf16x3": _capi.MATRIX_BF16X3}


def set_matrix_mode(mode, device=None):
    """How the frame-parallel matrix products of this process's handle on `device` contract
    (include/drnmf.h, DRNMF_MATRIX_*): 'f32' (exact-fp32 MFMA, the default) or 'bf16x3' (three bf16 planes
    per operand, six bf16 MFMAs per product, fp32 accumulate).  Returns the previous mode's name."""
    if mode not in MATRIX_MODES:
        raise ValueError("matrix mode must be one of %s" % sorted(MATRIX_MODES))
    dev = torch.cuda.current_device() if device is None else _dev_of(device)
    prev = get_matrix_mode(dev)
    _call("drnmf_set_matrix_mode", dev, MATRIX_MODES[mode], stream=False)
    return prev


def get_matrix_mode(device=None):
    L = _capi.lib()
    h = _capi.handle(torch.cuda.current_device() if device is None else _dev_of(device))
    return {v: k for k, v in MATRIX_MODES.items()}[L.drnmf_get_matrix_mode(h)]


def divide_a_by_aplusb(A, B):
    """exp(log(1e-7+A) - log(1e-7+A+B)) (custom_layers.py:41-45), elementwise."""
    dev = _dev_index(A)
    A, B = _f32c(A, "A"), _f32c(B, "B")
    if A.shape != B.shape:
        raise ValueError("A and B must have the same shape")
    out = torch.empty_like(A)
    _call("drnmf_divide_a_by_aplusb", dev, A.numel(), _capi.ptr(A), _capi.ptr(B), _capi.ptr(out))
    return out


def add(a, b):
    dev = _dev_index(a)
    a, b = _f32c(a, "a"), _f32c(b, "b")
    if a.shape != b.shape:
        raise ValueError("a and b must have the same shape")
    out = torch.empty_like(a)
    _call("drnmf_add", dev, a.numel(), _capi.ptr(a), _capi.ptr(b), _capi.ptr(out))
    return out


def loss_forward(y, w, x_raw=None, mask=None, A=None, Bn=None, hidden=None, l1_weight=0.0):
    """Validation loss sums {sum_rows w*loss_row, #rows with w != 0} (device tensor of 2 floats).
    mask given: mean_F (x_raw*mask - y)^2;  A, Bn, hidden given: the SNMF pretraining cost
    0.5 mean_F (A+Bn-y)^2 + l1_weight * mean_N |hidden| (enhance.py:1027-1035)."""
    dev = _dev_index(y)
    F = y.shape[-1]
    rows = y.numel() // F
    y, w = _f32c(y, "y"), _f32c(w, "w")
    if w.numel() != rows:
        raise ValueError("w must have one weight per row")
    sums = torch.empty(2, dtype=torch.float32, device=y.device)
    ws = torch.empty(_capi.lib().drnmf_loss_forward_workspace_bytes(rows), dtype=torch.uint8, device=y.device)
    if mask is not None:
        x_raw, mask = _f32c(x_raw, "x_raw"), _f32c(mask, "mask")
        _call("drnmf_loss_forward", dev, rows, F, 0, _capi.ptr(x_raw), _capi.ptr(mask), None, _capi.ptr(y),
              _capi.ptr(w), None, 0, 0, 0.0, _capi.ptr(sums), _capi.ptr(ws), ws.numel())
    else:
        A, Bn, hidden = _f32c(A, "A"), _f32c(Bn, "Bn"), _f32c(hidden, "hidden")
        N2 = hidden.shape[-1]
        _call("drnmf_loss_forward", dev, rows, F, 1, None, _capi.ptr(A), _capi.ptr(Bn), _capi.ptr(y), _capi.ptr(w),
              _capi.ptr(hidden), N2, N2, float(l1_weight), _capi.ptr(sums), _capi.ptr(ws), ws.numel())
    return sums


def ista_forward(X, W, H, lam1, alph, K, divergence="ed", beta=2.0):
    """Frame-parallel ISTA (enhance.py:402-456) in row layout: X [n,F], W [F,N], H [n,N] updated
    IN PLACE and returned."""
    dev = _dev_index(X)
    X, W = _f32c(X, "X"), _f32c(W, "W")
    n, F = X.shape
    N = W.shape[1]
    _given(H, (n, N), torch.float32, X.device, "H (updated in place)")
    if W.shape[0] != F:
        raise ValueError("shape mismatch: X %s W %s H %s" % (tuple(X.shape), tuple(W.shape),
                                                              tuple(H.shape)))
    nbytes = _capi.lib().drnmf_ista_workspace_bytes(n, F, N)
    ws = _workspace(nbytes, X.device)
    _call("drnmf_ista_forward", dev, n, F, N, int(K), DIVERGENCES[divergence], float(beta), float(lam1),
          float(alph), _capi.ptr(X), _capi.ptr(W), _capi.ptr(H), _capi.ptr(ws), nbytes)
    return H


def mu_forward(V, W, H, sparsity, n_iter, beta=2.0, want_irm=False):
    """SNMF inference by multiplicative updates, W fixed (sparse_nmf_gpu.m:163-173, 210-229) in
    row layout: V [n,F], W [F,N], H [n,N] (initial value in, result out, in place).
    Returns (H, Wn[, irm])."""
    dev = _dev_index(V)
    V, W = _f32c(V, "V"), _f32c(W, "W")
    n, F = V.shape
    N = W.shape[1]
    _given(H, (n, N), torch.float32, V.device, "H (updated in place)")
    if W.shape[0] != F:
        raise ValueError("shape mismatch: V %s W %s H %s" % (tuple(V.shape), tuple(W.shape),
                                                              tuple(H.shape)))
    Wn = torch.empty_like(W)
    irm = torch.empty((n, F), dtype=torch.float32, device=V.device) if want_irm else None
    nbytes = _capi.lib().drnmf_mu_workspace_bytes(n, F, N)
    ws = _workspace(nbytes, V.device)
    _call("drnmf_mu_forward", dev, n, F, N, int(n_iter), float(beta), float(sparsity), _capi.ptr(V), _capi.ptr(W),
          _capi.ptr(Wn), _capi.ptr(H), _capi.ptr(irm), _capi.ptr(ws), nbytes)
    return (H, Wn, irm) if want_irm else (H, Wn)


def snmf_mask_admitted(F, N, beta=2.0):
    """True when the tile kernel of `snmf_mask_forward` takes the shape (beta == 2, N <= 512)."""
    return bool(_capi.lib().drnmf_snmf_mask_admitted(int(F), int(N), float(beta)))


def snmf_mask_path(path, rows, F, N, beta=2.0):
    """'gemm' or 'tile': what `path` means for `rows` frame rows.  'auto' is the tile kernel when the shape is
    admitted and rows <= _capi.SNMF_TILE_AUTO_MAX_ROWS (the library's own rule for path = 0; measured: DESIGN.md
    section 6h)."""
    if path not in _capi.SNMF_PATHS:
        raise ValueError("path must be 'auto', 'gemm' or 'tile' (got %r)" % (path,))
    if path != "auto":
        return path
    return "tile" if snmf_mask_admitted(F, N, beta) and int(rows) <= _capi.SNMF_TILE_AUTO_MAX_ROWS else "gemm"


def snmf_mask_workspace(path, B, T, F, N, beta, device, have=None):
    """The workspace `snmf_mask_forward` needs for this call: None on the tile path, else a uint8 tensor of
    drnmf_snmf_mask_workspace_bytes -- `have` itself when it is large enough and on `device`.  The one place the
    path decision meets the sizing."""
    if snmf_mask_path(path, int(B) * int(T), F, N, beta) == "tile":
        return None
    return _workspace(_capi.lib().drnmf_snmf_mask_workspace_bytes(int(B), int(T), int(F), int(N)), device, have)


def _snmf_args(x, Wn, h_init, out, dict16=None):
    """The argument checks the SNMF family's forwards share -> (device index, x, Wn, h_init, out) with the three
    inputs contiguous float32 and out [B,T,F] (allocated when None).  dict16: checked against Wn when given."""
    if x.dim() != 3 or Wn.dim() != 2 or Wn.shape[0] != x.shape[2] or tuple(h_init.shape) != (Wn.shape[1],):
        raise ValueError("shape mismatch: x %s Wn %s h_init %s" % (tuple(x.shape), tuple(Wn.shape),
                                                                    tuple(h_init.shape)))
    if Wn.shape[1] % 2:
        raise ValueError("Wn must have an even number of atoms (speech and noise halves), got %d" % Wn.shape[1])
    B, T, F = x.shape
    N = Wn.shape[1]
    if dict16 is not None and (tuple(dict16.shape) != (F, (N + 31) // 32 * 32) or dict16.dtype != torch.float16 or
                               not dict16.is_contiguous()):
        raise ValueError("dict16 must be snmf_f16_pack_dict(Wn): contiguous float16 %s, got %s %s" %
                         ((F, (N + 31) // 32 * 32), dict16.dtype, tuple(dict16.shape)))
    dev = _dev_index(x)
    x, Wn, h_init = _f32c(x, "x"), _f32c(Wn, "Wn"), _f32c(h_init, "h_init")
    return dev, x, Wn, h_init, _out(out, (B, T, F), torch.float32, x.device)


def snmf_mask_forward(x, Wn, h_init, sparsity, n_iter, beta=2.0, power=1.0, mask_value=None, path="auto",
                      out=None, workspace=None):
    """The sparse-NMF baseline's inference on padded sequences (drnmf_snmf_mask_forward, enhance.py:838-852):
    x [B,T,F], Wn [F,N] with unit-norm columns, h_init [N] (the initial activation of every frame, in the
    normalised basis) -> mask [B,T,F]; frames whose bins all equal mask_value get a zero mask (None: no frame is
    masked).  path: 'auto', 'gemm' (drnmf_mu_forward's launches) or 'tile' (one launch, beta == 2 and N <= 512
    only: ValueError otherwise).  workspace: a uint8 tensor to use on the GEMM path (`snmf_mask_workspace`; allocated
    here when None or too small)."""
    if path not in _capi.SNMF_PATHS:
        raise ValueError("path must be 'auto', 'gemm' or 'tile' (got %r)" % (path,))
    dev, x, Wn, h_init, out = _snmf_args(x, Wn, h_init, out)
    B, T, F = x.shape
    N = Wn.shape[1]
    workspace = snmf_mask_workspace(path, B, T, F, N, beta, x.device, have=workspace)
    _call("drnmf_snmf_mask_forward", dev, B, T, F, N, int(n_iter), float(beta), float(sparsity), float(power),
          *_mask_pair(mask_value), _capi.ptr(x), _capi.ptr(Wn), _capi.ptr(h_init), _capi.ptr(out),
          _capi.SNMF_PATHS[path], _capi.ptr(workspace), 0 if workspace is None else workspace.numel())
    return out


def snmf_f16_admitted(F, N, beta=2.0):
    """True when the fp16-operand kernel of `snmf_f16_forward` takes the shape (beta == 2, N even, N <= 512)."""
    return bool(_capi.lib().drnmf_snmf_f16_admitted(int(F), int(N), float(beta)))


def snmf_f16_pack_dict(Wn, out=None):
    """Wn [F,N] float32 -> the dictionary as `snmf_f16_forward` reads it: float16 [F, N rounded up to 32], zero
    behind N (drnmf_snmf_f16_pack_dict)."""
    dev = _dev_index(Wn)
    Wn = _f32c(Wn, "Wn")
    if Wn.dim() != 2:
        raise ValueError("Wn must be [F, N], got %s" % (tuple(Wn.shape),))
    F, N = Wn.shape
    out = _out(out, (F, (N + 31) // 32 * 32), torch.float16, Wn.device)
    _call("drnmf_snmf_f16_pack_dict", dev, F, N, _capi.ptr(Wn), _capi.ptr(out), out.numel() * 2)
    return out


def snmf_f16_forward(x, dict16, Wn, h_init, sparsity, n_iter, power=1.0, mask_value=None, out=None):
    """`snmf_mask_forward`'s tile path (beta == 2) with the operands of the iteration's products rounded to fp16
    (drnmf_snmf_f16_forward): x [B,T,F], dict16 = snmf_f16_pack_dict(Wn), Wn [F,N] float32 with unit-norm columns
    (the numerator and the final mask read it), h_init [N] -> mask [B,T,F].  N even and at most 512: ValueError
    otherwise."""
    dev, x, Wn, h_init, out = _snmf_args(x, Wn, h_init, out, dict16=dict16)
    B, T, F = x.shape
    N = Wn.shape[1]
    _call("drnmf_snmf_f16_forward", dev, B, T, F, N, int(n_iter), float(sparsity), float(power),
          *_mask_pair(mask_value), _capi.ptr(x), _capi.ptr(dict16), _capi.ptr(Wn), _capi.ptr(h_init), _capi.ptr(out))
    return out


def snmf_kl_admitted(F, N):
    """True when the KL tile kernel of `snmf_kl_forward` takes the shape (2 <= N <= 512)."""
    return bool(_capi.lib().drnmf_snmf_kl_admitted(int(F), int(N)))


def snmf_kl_forward(x, Wn, h_init, sparsity, n_iter, power=1.0, mask_value=None, v_floor=None, out=None,
                    workspace=None):
    """The sparse-NMF baseline's inference under the KL cost (beta == 1) as one launch (drnmf_snmf_kl_forward,
    csrc/snmf_kl.hip): x [B,T,F], Wn [F,N] with unit-norm columns, h_init [N] in the normalised basis -> mask
    [B,T,F]; frames whose bins all equal mask_value get a zero mask (None: no frame is masked).  v_floor: None -- the
    reference's rule, zeros of V = x^power are raised to the smallest positive entry of THIS call's V
    (sparse_nmf_gpu.m:201-205); a positive finite number -- zeros are raised to that constant, and a frame's mask no
    longer depends on the frames it is run with.  N even and at most 512: ValueError otherwise.  workspace: a uint8
    tensor of drnmf_snmf_kl_workspace_bytes (the floor as the kernel reads it; allocated here when None or too
    small)."""
    if v_floor is not None and not (float(v_floor) > 0 and float(v_floor) < float("inf")):
        raise ValueError("v_floor must be None or a positive finite number (got %r)" % (v_floor,))
    dev, x, Wn, h_init, out = _snmf_args(x, Wn, h_init, out)
    B, T, F = x.shape
    N = Wn.shape[1]
    workspace = _workspace(_capi.lib().drnmf_snmf_kl_workspace_bytes(), x.device, workspace)
    _call("drnmf_snmf_kl_forward", dev, B, T, F, N, int(n_iter), float(sparsity), float(power),
          *_mask_pair(mask_value), _capi.ptr(x), _capi.ptr(Wn), _capi.ptr(h_init),
          0.0 if v_floor is None else float(v_floor), _capi.ptr(out), _capi.ptr(workspace), workspace.numel())
    return out


def snmf_adapt_admitted(F, N, beta=2.0):
    """True when `snmf_adapt_forward` takes the shape (beta == 2, 2 <= N <= 512)."""
    return bool(_capi.lib().drnmf_snmf_adapt_admitted(int(F), int(N), float(beta)))


def snmf_adapt_workspace(B, T, F, N, n_fixed, device, have=None):
    """The workspace `snmf_adapt_forward` needs for this call: a uint8 tensor of drnmf_snmf_adapt_workspace_bytes --
    `have` itself when it is large enough and on `device`.  ValueError for a shape the entry point refuses."""
    need = _capi.lib().drnmf_snmf_adapt_workspace_bytes(int(B), int(T), int(F), int(N), int(n_fixed))
    if need == 0:
        raise ValueError("snmf_adapt: shape B=%d T=%d F=%d N=%d n_fixed=%d is not taken (N even, 2 <= N <= %d, "
                         "0 <= n_fixed <= N)" % (B, T, F, N, n_fixed, _capi.SNMF_ADAPT_MAX_N))
    return _workspace(need, device, have)


def snmf_adapt_forward(x, Wn, hn, sparsity, n_iter, n_fixed, power=1.0, mask_value=None, workspace=None,
                       return_dictionaries=False, return_activations=False):
    """The noise-adaptive sparse-NMF baseline on padded sequences (drnmf_snmf_adapt_forward): every row of x [B,T,F]
    keeps the first n_fixed atoms of Wn [F,N] (unit-norm columns) and fits the others to its own valid frames for
    n_iter iterations, all frames starting from hn [N] -> mask [B,T,F].  return_dictionaries / return_activations
    append the rows' dictionaries [B,F,N] / activations [B,T,N] (normalised basis; 0 at masked frames).  beta == 2
    only; workspace: a uint8 tensor (`snmf_adapt_workspace`; allocated here when None or too small)."""
    dev, x, Wn, hn, out = _snmf_args(x, Wn, hn, None)
    B, T, F = x.shape
    N = Wn.shape[1]
    workspace = snmf_adapt_workspace(B, T, F, N, n_fixed, x.device, have=workspace)
    Wd = torch.empty((B, F, N), dtype=torch.float32, device=x.device) if return_dictionaries else None
    Ha = torch.empty((B, T, N), dtype=torch.float32, device=x.device) if return_activations else None
    _call("drnmf_snmf_adapt_forward", dev, B, T, F, N, int(n_fixed), int(n_iter), float(sparsity), float(power),
          *_mask_pair(mask_value), _capi.ptr(x), _capi.ptr(Wn), _capi.ptr(hn), _capi.ptr(out), _capi.ptr(Wd),
          _capi.ptr(Ha), _capi.ptr(workspace), workspace.numel())
    ret = (out,) + ((Wd,) if return_dictionaries else ()) + ((Ha,) if return_activations else ())
    return ret[0] if len(ret) == 1 else ret


class SNMFOnlineState(object):
    """The caller-owned state of `snmf_online_forward` (include/drnmf_snmf_online.h): `buf`, a uint8 device tensor of
    drnmf_snmf_online_state_bytes, and the shape it was sized for.  Made by `snmf_online_state`."""

    def __init__(self, buf, B, F, N, n0, block):
        self.buf, self.B, self.F, self.N, self.n0, self.block = buf, int(B), int(F), int(N), int(n0), int(block)

    @property
    def device(self):
        return self.buf.device

    def _shape(self):
        return self.B, self.F, self.N, self.n0, self.block


def snmf_online_admitted(F, N, beta=2.0, block=64):
    """True when `snmf_online_forward` takes the shape (beta == 2, N even, 2 <= N <= 512, block a multiple of 16 in
    16..256)."""
    return bool(_capi.lib().drnmf_snmf_online_admitted(int(F), int(N), float(beta), int(block)))


def snmf_online_reset(state, Wn, rows=None):
    """Every row of `state` -- or, with rows (B booleans), the rows marked -- back to its start: dictionary Wn [F,N]
    (unit-norm columns), statistics and count 0 (drnmf_snmf_online_reset)."""
    dev = _dev_index(state.buf)
    Wn = _f32c(Wn, "Wn")
    if tuple(Wn.shape) != (state.F, state.N) or Wn.device != state.device:
        raise ValueError("Wn must be [%d, %d] on %s, got %s on %s" % (state.F, state.N, state.device,
                                                                      tuple(Wn.shape), Wn.device))
    flags = None
    if rows is not None:
        flags = torch.as_tensor(np.asarray(rows, dtype=bool).astype(np.int32).reshape(-1)).to(state.device)
        if flags.numel() != state.B:
            raise ValueError("rows must have %d entries, got %d" % (state.B, flags.numel()))
    _call("drnmf_snmf_online_reset", dev, *state._shape(), _capi.ptr(Wn), _capi.ptr(flags), _capi.ptr(state.buf),
          state.buf.numel())
    return state


def snmf_online_state(B, F, N, n0, block, Wn, device):
    """A reset state of B streams for `snmf_online_forward`: every row's dictionary is Wn [F,N] (unit-norm columns),
    of which the first n0 atoms stay fixed; `block` valid frames make one update.  ValueError for a shape the entry
    points refuse."""
    need = _capi.lib().drnmf_snmf_online_state_bytes(int(B), int(F), int(N), int(n0), int(block))
    if need == 0:
        raise ValueError("snmf_online: shape B=%d F=%d N=%d n0=%d block=%d is not taken (N even, 2 <= N <= %d, "
                         "0 <= n0 <= N, block a multiple of 16 in 16..256)" %
                         (B, F, N, n0, block, _capi.SNMF_ONLINE_MAX_N))
    state = SNMFOnlineState(torch.empty(need, dtype=torch.uint8, device=device), B, F, N, n0, block)
    return snmf_online_reset(state, Wn)


def snmf_online_workspace(B, T, F, N, n0, block, device, have=None):
    """The workspace a `snmf_online_forward` call of T frames needs: a uint8 tensor of
    drnmf_snmf_online_workspace_bytes -- `have` itself when it is large enough and on `device`."""
    need = _capi.lib().drnmf_snmf_online_workspace_bytes(int(B), int(T), int(F), int(N), int(n0), int(block))
    if need == 0:
        raise ValueError("snmf_online: shape B=%d T=%d F=%d N=%d n0=%d block=%d is not taken" %
                         (B, T, F, N, n0, block))
    return _workspace(need, device, have)


def snmf_online_forward(x, h_init, sparsity, n_iter, n0, state, w_iter=1, forget=1.0, power=1.0, mask_value=None,
                        workspace=None, out=None, return_h=False):
    """The online noise-adaptive sparse-NMF baseline (drnmf_snmf_online_forward): x [B,T,F] holds the next T frames
    of the B streams of `state` (masked frames where a stream has fewer) -> mask [B,T,F], and with return_h the
    activations [B,T,N] (0 at masked frames).  A valid frame is decomposed for n_iter iterations from h_init [N] on
    the dictionary its row had when the frame's block began; every full block of state.block valid frames moves the
    row's atoms from n0 on (w_iter updates from the statistics, which decay by `forget` per block).  The masks, the
    activations and the state do not depend on how a row's frames are cut into calls."""
    if x.dim() != 3 or tuple(h_init.shape) != (state.N,) or x.shape[2] != state.F or x.shape[0] != state.B:
        raise ValueError("shape mismatch: x %s h_init %s for a state of B=%d F=%d N=%d" %
                         (tuple(x.shape), tuple(h_init.shape), state.B, state.F, state.N))
    if int(n0) != state.n0:
        raise ValueError("n0 = %d, the state was made for n0 = %d" % (int(n0), state.n0))
    dev = _dev_index(x)
    x, h_init = _f32c(x, "x"), _f32c(h_init, "h_init")
    B, T, F = x.shape
    out = _out(out, (B, T, F), torch.float32, x.device)
    Ha = torch.empty((B, T, state.N), dtype=torch.float32, device=x.device) if return_h else None
    if T == 0:
        return (out, Ha) if return_h else out
    workspace = snmf_online_workspace(B, T, F, state.N, state.n0, state.block, x.device, have=workspace)
    _call("drnmf_snmf_online_forward", dev, B, T, F, state.N, state.n0, state.block, int(n_iter), int(w_iter),
          float(sparsity), float(forget), float(power), *_mask_pair(mask_value), _capi.ptr(x), _capi.ptr(h_init),
          _capi.ptr(out), _capi.ptr(Ha), _capi.ptr(state.buf), state.buf.numel(), _capi.ptr(workspace),
          workspace.numel())
    return (out, Ha) if return_h else out


def _snmf_online_read(state, want_w, want_stats):
    dev = _dev_index(state.buf)
    B, F, N, n0, _ = state._shape()
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=state.device)
    W = new(B, F, N) if want_w else None
    counts = torch.empty((B,), dtype=torch.int64, device=state.device) if want_w else None
    A = new(B, N, N - n0) if want_stats else None
    Bm = new(B, F, N - n0) if want_stats else None
    _call("drnmf_snmf_online_read", dev, *state._shape(), _capi.ptr(state.buf), state.buf.numel(), _capi.ptr(W),
          _capi.ptr(counts), _capi.ptr(A), _capi.ptr(Bm))
    return W, counts, A, Bm


def snmf_online_dictionaries(state):
    """(the streams' dictionaries [B,F,N] float32, the valid frames each has seen [B] int64), copied out of `state`
    (drnmf_snmf_online_read)."""
    return _snmf_online_read(state, True, False)[:2]


def snmf_online_statistics(state):
    """(A [B,N,N-n0], Bm [B,F,N-n0]): the streams' sufficient statistics, copied out of `state`."""
    return _snmf_online_read(state, False, True)[2:]


def stft_frames(nsampl, N, hop):
    return int(_capi.lib().drnmf_stft_frames(int(nsampl), int(N), int(hop)))


def stft_mag(pcm, N=1024, hop=None):
    """pcm [n_sig, nsampl] int16 (scaled by 1/32768, util.py:29-35) or float32 ->
    |STFT| [n_sig, n_frames, N/2+1] with the sqrt-Hann window (audio_dataset.py:194)."""
    dev = _dev_index(pcm)
    if hop is None:
        hop = N // 2
    if pcm.dim() == 1:
        pcm = pcm[None]
    if pcm.dtype not in (torch.int16, torch.float32):
        raise ValueError("pcm must be int16 or float32")
    pcm = pcm.contiguous()
    n_sig, nsampl = pcm.shape
    nf = stft_frames(nsampl, N, hop)
    mag = torch.empty((n_sig, nf, N // 2 + 1), dtype=torch.float32, device=pcm.device)
    _call("drnmf_stft_mag", dev, n_sig, nsampl, int(N), int(hop), int(pcm.dtype == torch.int16), _capi.ptr(pcm),
          _capi.ptr(mag))
    return mag


class SnmfTrainer(object):
    """Device state of one sparse-NMF training problem (one chunk of frames): V [n,F] rows,
    W [F,N], H [n,N].  `step()` runs one iteration of sparse_nmf_gpu.m:210-281 and returns a device
    tensor obj = [div, cost]."""

    def __init__(self, V, W, H, beta=2.0):
        self.dev = _dev_index(V)
        self.V, self.W, self.H = _f32c(V, "V"), _f32c(W, "W").clone(), _f32c(H, "H").clone()
        self.n, self.F = self.V.shape
        self.N = self.W.shape[1]
        if self.W.shape[0] != self.F or tuple(self.H.shape) != (self.n, self.N):
            raise ValueError("shape mismatch: V %s W %s H %s" % (tuple(V.shape), tuple(W.shape),
                                                                  tuple(H.shape)))
        self.beta = float(beta)
        self.nbytes = _capi.lib().drnmf_snmf_train_workspace_bytes(self.n, self.F, self.N)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=V.device)
        _call("drnmf_snmf_train_init", self.dev, self.n, self.F, self.N, self.beta, _capi.ptr(self.V),
              _capi.ptr(self.W), _capi.ptr(self.H), _capi.ptr(self.ws), self.nbytes)

    def step(self, sparsity, w_update_mask=None, update_w=True, obj=None):
        """obj: a 2-element float32 device tensor (e.g. a row of a preallocated [max_iter, 2] log)
        that receives [div, cost]; allocated here when None.  Nothing is synchronised."""
        obj = _out(obj, (2,), torch.float32, self.V.device, "obj")
        m = None
        if w_update_mask is not None:
            m = w_update_mask.to(device=self.V.device, dtype=torch.uint8).contiguous()
            if m.numel() != self.N:
                raise ValueError("w_update_mask must have N entries")
        _call("drnmf_snmf_train_step", self.dev, self.n, self.F, self.N, self.beta, float(sparsity),
              _capi.ptr(self.W), _capi.ptr(self.H), _capi.ptr(m), int(bool(update_w)), _capi.ptr(obj),
              _capi.ptr(self.ws), self.nbytes)
        return obj


def stft(pcm, N=1024, hop=None, want_mag=False):
    """Complex STFT (reference stack convention: conjugated spectrum, util.py:195,351).
    Returns (re, im[, mag]) each [n_sig, n_frames, N/2+1]."""
    dev = _dev_index(pcm)
    if hop is None:
        hop = N // 2
    if pcm.dim() == 1:
        pcm = pcm[None]
    if pcm.dtype not in (torch.int16, torch.float32):
        raise ValueError("pcm must be int16 or float32")
    pcm = pcm.contiguous()
    n_sig, nsampl = pcm.shape
    nf = stft_frames(nsampl, N, hop)
    shape = (n_sig, nf, N // 2 + 1)
    re = torch.empty(shape, dtype=torch.float32, device=pcm.device)
    im = torch.empty(shape, dtype=torch.float32, device=pcm.device)
    mag = torch.empty(shape, dtype=torch.float32, device=pcm.device) if want_mag else None
    _call("drnmf_stft", dev, n_sig, nsampl, int(N), int(hop), int(pcm.dtype == torch.int16), _capi.ptr(pcm),
          _capi.ptr(re), _capi.ptr(im), _capi.ptr(mag))
    return (re, im, mag) if want_mag else (re, im)


def istft_masked(re, im, mask, nsampl, N, hop):
    """y [n_sig, nsampl] = istft_noDiv(mask * (re + i im)) with the sqrt-Hann synthesis window
    (audio_dataset.py:267-278; util.py:48-169, 203-226).  mask may be None."""
    dev = _dev_index(re)
    re, im = _f32c(re, "re"), _f32c(im, "im")
    n_sig, nf, F = re.shape
    if F != N // 2 + 1:
        raise ValueError("re/im have %d bins, N=%d needs %d" % (F, N, N // 2 + 1))
    if mask is not None:
        mask = _f32c(mask, "mask")
        if tuple(mask.shape) != tuple(re.shape):
            raise ValueError("mask shape %s != spectrum shape %s" % (tuple(mask.shape),
                                                                     tuple(re.shape)))
    y = torch.empty((n_sig, int(nsampl)), dtype=torch.float32, device=re.device)
    nbytes = _capi.lib().drnmf_istft_workspace_bytes(n_sig, nf, int(N))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=re.device)
    _call("drnmf_istft_masked", dev, n_sig, nf, int(nsampl), int(N), int(hop), _capi.ptr(re), _capi.ptr(im),
          _capi.ptr(mask), _capi.ptr(y), _capi.ptr(ws), nbytes)
    return y


def snr_db(est, ref):
    """Raw SNR per signal (score_audio.m:209)."""
    dev = _dev_index(est)
    est, ref = _f32c(est, "est"), _f32c(ref, "ref")
    if est.dim() == 1:
        est, ref = est[None], ref[None]
    n_sig, nsampl = est.shape
    out = torch.empty(n_sig, dtype=torch.float32, device=est.device)
    _call("drnmf_snr", dev, n_sig, nsampl, _capi.ptr(est), _capi.ptr(ref), _capi.ptr(out))
    return out


def toeplitz_solve(r, d):
    """Solve the symmetric Toeplitz systems Toeplitz(r[k]) c[k] = d[k] on the device (Levinson-Durbin, fp64;
    include/drnmf_sdr.h).  r, d: device float64 [n_sys, n] (or 1-D), n <= 2048.  Returns (c, info): c like r,
    info int32 [n_sys] -- 0 solved, 1 r[0] <= 0 or not finite (c = 0), 2 + k the recursion stopped at step k."""
    dev = _dev_index(r)
    if r.dtype != torch.float64 or d.dtype != torch.float64 or r.shape != d.shape or r.device != d.device:
        raise ValueError("toeplitz_solve: r and d must be float64 tensors of one shape on one device")
    one = r.dim() == 1
    r2, d2 = (r[None], d[None]) if one else (r, d)
    if r2.dim() != 2 or r2.shape[0] < 1:
        raise ValueError("toeplitz_solve: r and d must be [n_sys, n] with n_sys >= 1")
    r2, d2 = r2.contiguous(), d2.contiguous()
    n_sys, n = r2.shape
    c = torch.empty_like(r2)
    info = torch.empty(n_sys, dtype=torch.int32, device=r2.device)
    _call("drnmf_toeplitz_solve", dev, n_sys, n, _capi.ptr(r2), _capi.ptr(d2), _capi.ptr(c), _capi.ptr(info))
    return (c[0] if one else c), info


SDR_SOLVERS = ("host", "device")


def _sdr_lengths(lengths, n_sig, width, dev):
    """As _ragged_lengths, with 0 allowed (a row of length 0 is a silent pair).  A device tensor is not read
    back: the kernels clamp it into [0, width]."""
    if lengths is None:
        return None
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        ld = lengths.to(device=dev, dtype=torch.int64).contiguous().reshape(-1)
        if ld.numel() != n_sig:
            raise ValueError("sdr_db: lengths has %d entries for %d signals" % (ld.numel(), n_sig))
        return ld
    lh = lengths.detach().cpu().numpy() if isinstance(lengths, torch.Tensor) else lengths
    lh = np.ascontiguousarray(np.asarray(lh, dtype=np.int64).reshape(-1))
    if lh.shape[0] != n_sig:
        raise ValueError("sdr_db: lengths has %d entries for %d signals" % (lh.shape[0], n_sig))
    if n_sig and (lh.min() < 0 or lh.max() > width):
        raise ValueError("sdr_db: every length must lie in [0, %d] (got %d .. %d)" % (width, lh.min(), lh.max()))
    return torch.from_numpy(lh).to(dev)


def sdr_ragged_enqueue(est, ref, lengths_dev, flen, out, coef=None, energies=None, r=None, d=None, info=None,
                       workspace=None):
    """drnmf_sdr_ragged on tensors the caller owns and has checked: enqueues, reads nothing back."""
    dev = _dev_index(est)
    n_sig, stride = est.shape
    nbytes = _capi.lib().drnmf_sdr_ragged_workspace_bytes(n_sig, stride, int(flen))
    workspace = _workspace(max(nbytes, 256), est.device, workspace)
    _call("drnmf_sdr_ragged", dev, n_sig, stride, _capi.ptr(lengths_dev), int(flen), _capi.ptr(est), _capi.ptr(ref),
          _capi.ptr(out), _capi.ptr(coef), _capi.ptr(energies), _capi.ptr(r), _capi.ptr(d), _capi.ptr(info),
          _capi.ptr(workspace), workspace.numel())


def sdr_db(est, ref, flen=512, return_parts=False, lengths=None, solver="host"):
    """SDR per signal as `bss_eval_sources(xest', xref')` computes it for one source
    (score_audio.m:206; BSS Eval 3.0, 512-tap time-invariant filters).  Correlations, the
    projection and the energies run on the device in fp64; the flen x flen Toeplitz normal
    equations are solved on the host (numpy fp64), one system per signal.

    solver="device" (include/drnmf_sdr.h): the systems are solved on the device too (Levinson-Durbin) and the
    whole score is only enqueued -- no host round trip.  lengths (host ints or a tensor, each in [0, width]; device
    solver only): row i is scored over its first lengths[i] samples, whatever lies behind them; a row's numbers
    are bitwise the same in any batch.  return_parts=True then returns (sdr, coef, energies, info), info as
    `toeplitz_solve` returns it."""
    if solver not in SDR_SOLVERS:
        raise ValueError("sdr_db: solver must be one of %s (got %r)" % (SDR_SOLVERS, solver))
    if lengths is not None and solver == "host":
        raise ValueError("sdr_db: lengths= needs solver='device' (the host solver scores whole rows)")
    di = _dev_index(est)
    est, ref = _f32c(est, "est"), _f32c(ref, "ref")
    if est.dim() == 1:
        est, ref = est[None], ref[None]
    if est.shape != ref.shape:
        raise ValueError("est and ref must have the same shape")
    n_sig, nsampl = est.shape
    if solver == "device":
        if est.dim() != 2 or n_sig < 1 or nsampl < 1 or ref.device != est.device:
            raise ValueError("sdr_db: est and ref must be non-empty [n_sig, n] tensors on one device")
        dev = est.device
        ld = _sdr_lengths(lengths, n_sig, nsampl, dev)
        out = torch.empty(n_sig, dtype=torch.float32, device=dev)
        coef = en = info = None
        if return_parts:
            coef = torch.empty((n_sig, int(flen)), dtype=torch.float64, device=dev)
            en = torch.empty((n_sig, 2), dtype=torch.float64, device=dev)
            info = torch.empty(n_sig, dtype=torch.int32, device=dev)
        sdr_ragged_enqueue(est, ref, ld, flen, out, coef=coef, energies=en, info=info)
        return (out, coef, en, info) if return_parts else out
    dev = est.device
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    r, d, coef, en = f64(n_sig, flen), f64(n_sig, flen), f64(n_sig, flen), f64(n_sig, 2)
    out = torch.empty(n_sig, dtype=torch.float32, device=dev)
    ws = _workspace(max(_capi.lib().drnmf_sdr_workspace_bytes(n_sig, nsampl, flen), 256), dev)
    _call("drnmf_sdr_corr", di, n_sig, nsampl, flen, _capi.ptr(est), _capi.ptr(ref), _capi.ptr(r), _capi.ptr(d),
          _capi.ptr(ws), ws.numel())
    rh, dh = r.cpu().numpy(), d.cpu().numpy()
    idx = np.abs(np.arange(flen)[:, None] - np.arange(flen)[None, :])
    ch = np.empty_like(dh)
    for i in range(n_sig):
        G = rh[i][idx]
        try:
            ch[i] = np.linalg.solve(G, dh[i])
        except np.linalg.LinAlgError:          # silent reference: any solution of G c = d
            ch[i] = np.linalg.lstsq(G, dh[i], rcond=None)[0]
    coef.copy_(torch.from_numpy(ch))
    _call("drnmf_sdr_project", di, n_sig, nsampl, flen, _capi.ptr(est), _capi.ptr(ref), _capi.ptr(coef),
          _capi.ptr(en), _capi.ptr(out), _capi.ptr(ws), ws.numel())
    return (out, coef, en) if return_parts else out


def to_int16_wav(x):
    """util.wavwrite's float32 -> int16 conversion (util.py:37-45): divide by max|x| if it exceeds
    1, scale by 32767, truncate toward zero (numpy int16 cast)."""
    dev = _dev_index(x)
    x = _f32c(x, "x")
    out = torch.empty(x.shape, dtype=torch.int16, device=x.device)
    ws = torch.empty(_capi.lib().drnmf_wav_int16_workspace_bytes(), dtype=torch.uint8, device=x.device)
    _call("drnmf_wav_int16", dev, x.numel(), _capi.ptr(x), _capi.ptr(out), _capi.ptr(ws), ws.numel())
    return out


# ---- ragged batches: STFT into the model's layout, masked inverse, int16 per row (include/drnmf_enhance.h) ----
def _ragged_lengths(lengths, n_sig, width, dev, what):
    """lengths (host ints, numpy or a tensor on any device) -> (host int64 numpy, device int64 tensor); every
    length must lie in [1, width]."""
    if isinstance(lengths, torch.Tensor):
        ld = lengths.to(device=dev, dtype=torch.int64).contiguous().reshape(-1) if lengths.is_cuda else None
        lh = lengths.detach().cpu().numpy()
    else:
        ld, lh = None, lengths
    lh = np.ascontiguousarray(np.asarray(lh, dtype=np.int64).reshape(-1))
    if lh.shape[0] != n_sig:
        raise ValueError("%s: lengths has %d entries for %d signals" % (what, lh.shape[0], n_sig))
    if n_sig and (lh.min() < 1 or lh.max() > width):
        raise ValueError("%s: every length must lie in [1, %d] (got %d .. %d)" % (what, width, lh.min(), lh.max()))
    if ld is None:
        ld = torch.from_numpy(lh).to(dev)
    return lh, ld


def _ragged_index(sig_index, n_sig, dev, what):
    if sig_index is None:
        return torch.arange(n_sig, dtype=torch.int32, device=dev)
    if isinstance(sig_index, torch.Tensor):
        ih = sig_index.detach().cpu().numpy()
    else:
        ih = sig_index
    ih = np.ascontiguousarray(np.asarray(ih, dtype=np.int64).reshape(-1))
    if ih.shape[0] < 1 or ih.min() < 0 or ih.max() >= n_sig:
        raise ValueError("%s: sig_index must hold at least one index, all in [0, %d)" % (what, n_sig))
    if isinstance(sig_index, torch.Tensor) and sig_index.is_cuda and sig_index.dtype == torch.int32:
        return sig_index.contiguous().reshape(-1)
    return torch.from_numpy(ih.astype(np.int32)).to(dev)


def ragged_out_lengths(lengths, N, hop, crop=False):
    """Samples of each row's reconstruction: hop * (n_frames - 1) - N, which is ceil(len / hop) * hop when hop
    divides N (what reconstruct_x returns); crop=True: at most the row's own length."""
    lh = np.asarray(lengths, dtype=np.int64).reshape(-1)
    nf = 1 + (-(-lh // hop) * hop + N) // hop
    n = np.maximum(hop * (nf - 1) - N, 0)
    return np.minimum(n, lh) if crop else n


def stft_ragged_enqueue(pcm, lengths_dev, sig_index_dev, T, N, hop, mask_value, x, re, im):
    """drnmf_stft_ragged on tensors the caller owns and has checked: enqueues, reads nothing back."""
    dev = _dev_index(pcm)
    n_sig, stride = pcm.shape
    _call("drnmf_stft_ragged", dev, n_sig, stride, _capi.ptr(lengths_dev), sig_index_dev.numel(),
          _capi.ptr(sig_index_dev), int(T), int(N), int(hop), int(pcm.dtype == torch.int16), float(mask_value),
          _capi.ptr(pcm), _capi.ptr(x), _capi.ptr(re), _capi.ptr(im))


def stft_ragged(pcm, lengths, sig_index=None, T=None, N=512, hop=None, mask_value=-1.0):
    """STFT of a ragged batch straight into the model's layout.  pcm [n_sig, stride] int16 (scaled by 1/32768) or
    float32 on the device, row i valid up to lengths[i] (host ints or a tensor, each in [1, stride]); sig_index [b]
    (default: every row in order): slab row k is signal sig_index[k]; T: the slab's frame capacity (default: the
    longest of the slab).  Returns (x, re, im, n_frames): x [b, T, N/2+1] the magnitude with mask_value in every
    bin of the frames behind a row's own n_frames[k] (audio_dataset.py:144-146); re, im as `stft` returns them,
    rows behind n_frames[k] unspecified; n_frames int64 numpy [b] = stft_frames(length, N, hop)."""
    if hop is None:
        hop = N // 2
    if pcm.dim() == 1:
        pcm = pcm[None]
    if pcm.dim() != 2 or pcm.dtype not in (torch.int16, torch.float32):
        raise ValueError("stft_ragged: pcm must be [n_sig, stride] int16 or float32")
    dev = pcm.device
    _dev_index(pcm)
    pcm = pcm.contiguous()
    n_sig, stride = pcm.shape
    if n_sig < 1 or stride < 1 or int(hop) < 1:
        raise ValueError("stft_ragged: empty batch or hop < 1")
    lh, ld = _ragged_lengths(lengths, n_sig, stride, dev, "stft_ragged")
    idx = _ragged_index(sig_index, n_sig, dev, "stft_ragged")
    ih = np.arange(n_sig) if sig_index is None else idx.cpu().numpy()
    nf = np.array([stft_frames(int(lh[i]), N, hop) for i in ih], dtype=np.int64)
    if T is None:
        T = int(nf.max())
    if int(T) < int(nf.max()):
        raise ValueError("stft_ragged: T = %d is below the slab's longest row (%d frames)" % (T, nf.max()))
    shape = (idx.numel(), int(T), N // 2 + 1)
    x = torch.empty(shape, dtype=torch.float32, device=dev)
    re, im = torch.empty_like(x), torch.empty_like(x)
    stft_ragged_enqueue(pcm, ld, idx, T, N, hop, mask_value, x, re, im)
    return x, re, im, nf


# ---- training tensors from waveform pairs (include/drnmf_dataset.h) -----------------------------------------
def stft_pair_chunks_enqueue(pcm_x, pcm_y, len_x_dev, len_y_dev, table_dev, T, N, hop, transform, mask_value,
                             x, y, w):
    """drnmf_stft_pair_chunks on tensors the caller owns and has checked: enqueues, reads nothing back."""
    _call("drnmf_stft_pair_chunks", _dev_index(pcm_x), pcm_x.shape[0], pcm_x.shape[1], pcm_y.shape[1],
          _capi.ptr(len_x_dev), _capi.ptr(len_y_dev), table_dev.shape[0], _capi.ptr(table_dev), int(T), int(N),
          int(hop), int(pcm_x.dtype == torch.int16), _capi.TRANSFORMS[transform], float(mask_value),
          _capi.ptr(pcm_x), _capi.ptr(pcm_y), _capi.ptr(x), _capi.ptr(y), _capi.ptr(w))


def stft_pair_target_enqueue(pcm_x, pcm_y, len_x_dev, len_y_dev, table_dev, T, N, hop, transform, target,
                              mask_value, x, y, w):
    """drnmf_stft_pair_chunks_target (include/drnmf_target.h) on tensors the caller owns and has checked:
    stft_pair_chunks_enqueue with y = the 'mag' / 'psa' / 'tpsa' target.  Enqueues, reads nothing back."""
    _call("drnmf_stft_pair_chunks_target", _dev_index(pcm_x), pcm_x.shape[0], pcm_x.shape[1], pcm_y.shape[1],
          _capi.ptr(len_x_dev), _capi.ptr(len_y_dev), table_dev.shape[0], _capi.ptr(table_dev), int(T), int(N),
          int(hop), int(pcm_x.dtype == torch.int16), _capi.TRANSFORMS[transform], _capi.TARGETS[target],
          float(mask_value), _capi.ptr(pcm_x), _capi.ptr(pcm_y), _capi.ptr(x), _capi.ptr(y), _capi.ptr(w))


def stft_pair_frames_enqueue(pcm_x, pcm_y, len_x_dev, len_y_dev, row0_dev, N, hop, transform, x_frames,
                             y_frames):
    """drnmf_stft_pair_frames on tensors the caller owns and has checked: enqueues, reads nothing back."""
    _call("drnmf_stft_pair_frames", _dev_index(pcm_x), pcm_x.shape[0], pcm_x.shape[1], pcm_y.shape[1],
          _capi.ptr(len_x_dev), _capi.ptr(len_y_dev), _capi.ptr(row0_dev), x_frames.shape[0], int(N), int(hop),
          int(pcm_x.dtype == torch.int16), _capi.TRANSFORMS[transform], _capi.ptr(pcm_x), _capi.ptr(pcm_y),
          _capi.ptr(x_frames), _capi.ptr(y_frames))


def _check_wav_pairs(noisy, clean, N, hop, transform, what):
    """Host-side checks of a list of (noisy, clean) waveform pairs, before the device is touched.  Returns
    (noisy rows, clean rows, numpy dtype, frame counts of the clean side)."""
    N, hop = int(N), int(hop)
    if transform not in _capi.TRANSFORMS:
        raise ValueError("%s: transform must be 'mag' or 'logmag' (got %r)" % (what, transform))
    if N < 64 or N > 4096 or N & (N - 1) or hop < 1:
        raise ValueError("%s: N = %d must be a power of two in [64, 4096] and hop = %d positive" % (what, N, hop))
    rx, ry = [np.asarray(v) for v in noisy], [np.asarray(v) for v in clean]
    if len(rx) != len(ry):
        raise ValueError("%s: %d noisy waveforms for %d clean ones" % (what, len(rx), len(ry)))
    if not rx:
        raise ValueError("%s: no waveforms" % what)
    dt = rx[0].dtype
    if dt not in (np.dtype('int16'), np.dtype('float32')):
        raise ValueError("%s: waveforms must be int16 or float32 (got %s)" % (what, dt))
    for v in rx + ry:
        if v.ndim != 1 or v.dtype != dt or v.shape[0] < 1:
            raise ValueError("%s: every waveform must be a non-empty 1-D %s array" % (what, dt))
    frames = lambda n: -(-n // hop) + N // hop + 1                 # drnmf_stft_frames
    nf = np.array([frames(v.shape[0]) for v in ry], dtype=np.int64)
    for i, v in enumerate(rx):
        if frames(v.shape[0]) < nf[i]:
            # the case the reference means to refuse (audio_dataset.py:239-240) but does not
            raise ValueError("%s: noisy waveform %d has %d frames, fewer than its clean one's %d"
                             % (what, i, frames(v.shape[0]), nf[i]))
    return rx, ry, dt, nf


def _upload_wav_side(rows, dt, dev):
    """One pinned upload of one side: lengths [n] int64 | samples [n][stride].  Returns (pcm, lengths) on the
    device.  The samples behind a row's own length are left as they are: the kernels never read them."""
    n = len(rows)
    lens = np.array([v.shape[0] for v in rows], dtype=np.int64)
    stride = int(lens.max())
    off = -(-(8 * n) // 16) * 16
    host = torch.empty(off + n * stride * dt.itemsize, dtype=torch.uint8, pin_memory=True)
    hn = host.numpy()
    hn[:8 * n].view(np.int64)[:] = lens
    pk = hn[off:].view(dt).reshape(n, stride)
    for i, v in enumerate(rows):
        pk[i, :v.shape[0]] = v
    d = host.to(dev, non_blocking=True)
    pcm = d[off:].view(torch.int16 if dt == np.dtype('int16') else torch.float32).view(n, stride)
    return pcm, d[:8 * n].view(torch.int64)


def _upload_pinned(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)


def _check_target(target, transform, what):
    """The training target of include/drnmf_target.h against the transform, before the device is touched."""
    if target not in _capi.TARGETS:
        raise ValueError("%s: target must be 'mag', 'psa' or 'tpsa' (got %r)" % (what, target))
    if target != 'mag' and transform != 'mag':
        raise ValueError("%s: target %r is defined for transform 'mag' only (got %r)" % (what, target, transform))


def wavs_to_tensors(noisy, clean, N=512, hop=128, maxlen=None, transform='mag', mask_value=None, device=None,
                    target='mag'):
    """The reference's load_data (audio_dataset.py:199-264: STFT of every noisy and clean file, the noisy stack
    clipped to the clean one, the transform, get_padded_data_matrix) on the device: lists of 1-D int16 (scaled
    by 1/32768) or float32 numpy arrays in, (x, y, w) out as device tensors [n_seq, T, F], [n_seq, T, F] and
    [n_seq, T] -- what `fit(x, y, sample_weight=w)` takes.  Every utterance is cut into consecutive sequences of
    at most maxlen frames (data.sequence_table_from_lengths; None: one sequence per utterance), padded with
    mask_value (default: data.get_mask_value for the transform) and weighted 1 / 0.  The clean side decides an
    utterance's frame count; a noisy signal with FEWER frames than its clean one raises ValueError, as do lists
    of different lengths and empty lists.  One pinned upload per side and one of the table, one launch
    sequence, no download and no synchronisation.

    target: what y holds in a valid frame.  'mag': the clean magnitude, as the reference trains.  'psa': the
    phase-sensitive target p = |S| cos(theta_S - theta_X) (Erdogan et al., ICASSP 2015), the clean magnitude
    projected on the noisy phase the enhanced signal is put back on; it may be negative and may exceed x.
    'tpsa': p clipped to [0, x], what a mask in [0, 1] can reach.  p is 0 where the noisy bin is 0.  x and w do not
    depend on the target.  'psa' and 'tpsa' need transform='mag' (ValueError otherwise)."""
    from . import data
    _check_target(target, transform, "wavs_to_tensors")
    rx, ry, dt, nf = _check_wav_pairs(noisy, clean, N, hop, transform, "wavs_to_tensors")
    table, T = data.sequence_table_from_lengths(nf, maxlen)
    if mask_value is None:
        mask_value = data.get_mask_value(dict(transform_x=transform, transform_y=transform))
    dev = torch.device('cuda' if device is None else device)
    dev = torch.device('cuda', _dev_of(dev))
    with torch.cuda.device(dev):
        pcm_x, len_x = _upload_wav_side(rx, dt, dev)
        pcm_y, len_y = _upload_wav_side(ry, dt, dev)
        table_d = _upload_pinned(table, dev)
        n_seq, F = table.shape[0], int(N) // 2 + 1
        x = torch.empty((n_seq, T, F), dtype=torch.float32, device=dev)
        y = torch.empty_like(x)
        w = torch.empty((n_seq, T), dtype=torch.float32, device=dev)
        if target == 'mag':
            stft_pair_chunks_enqueue(pcm_x, pcm_y, len_x, len_y, table_d, T, N, hop, transform, mask_value, x, y, w)
        else:
            stft_pair_target_enqueue(pcm_x, pcm_y, len_x, len_y, table_d, T, N, hop, transform, target, mask_value,
                                     x, y, w)
    return x, y, w


def wavs_to_frames(noisy, clean, N, hop, transform='mag'):
    """The unpadded frames of both sides, as the reference gets them by masked_seqs_to_frames of load_data's
    tensors (enhance.py:772-813), in the row layout `mu_forward` and the dictionary trainer take: (x_frames,
    y_frames), each [total_frames, F] on the current device, utterance after utterance.  Arguments and errors
    as `wavs_to_tensors`."""
    rx, ry, dt, nf = _check_wav_pairs(noisy, clean, N, hop, transform, "wavs_to_frames")
    dev = torch.device('cuda', torch.cuda.current_device())
    total = int(nf.sum())
    pcm_x, len_x = _upload_wav_side(rx, dt, dev)
    pcm_y, len_y = _upload_wav_side(ry, dt, dev)
    row0 = _upload_pinned(np.cumsum(nf) - nf, dev)
    xf = torch.empty((total, int(N) // 2 + 1), dtype=torch.float32, device=dev)
    yf = torch.empty_like(xf)
    stft_pair_frames_enqueue(pcm_x, pcm_y, len_x, len_y, row0, N, hop, transform, xf, yf)
    return xf, yf


# ---- rate conversion on the device (include/drnmf_resample.h) ------------------------------------------------
RESAMPLE_MAX_PQ, RESAMPLE_TILE = _capi.RESAMPLE_MAX_PQ, _capi.RESAMPLE_TILE
RESAMPLE_NZ, RESAMPLE_BETA = _capi.RESAMPLE_NZ, _capi.RESAMPLE_BETA


def resample_rate(fs_in, fs_out):
    """(p, q) with p / q = fs_out / fs_in reduced (drnmf_resample_rate).  ValueError for a rate that is not a positive
    whole number and for max(p, q) > RESAMPLE_MAX_PQ = 640."""
    for fs in (fs_in, fs_out):
        if isinstance(fs, bool) or not isinstance(fs, (int, float, np.integer, np.floating)) or \
                not (np.isfinite(fs) and 0 < fs < 2 ** 62 and fs == int(fs)):
            raise ValueError("resample: a rate must be a positive whole number (got %r)" % (fs,))
    p, q = C.c_int32(), C.c_int32()
    if _capi.lib().drnmf_resample_rate(int(fs_in), int(fs_out), C.byref(p), C.byref(q)) != _capi.OK:
        raise ValueError("resample: %r -> %r reduces to p / q with max(p, q) > %d" % (fs_in, fs_out, RESAMPLE_MAX_PQ))
    return p.value, q.value


def resample_out_lengths(lengths, fs_in, fs_out):
    """ceil(n p / q) for every n of `lengths`, int64, on the host."""
    p, q = resample_rate(fs_in, fs_out)
    n = np.asarray(lengths, dtype=np.int64)
    if (n < 0).any():
        raise ValueError("resample_out_lengths: a length is negative")
    return -(-n * p // q)


def _resample_filter_shape(p, q, nz):
    """(L, tile) of the kernel for a reduced rate: the filter's taps (0 for p == q == 1) and the outputs per
    workgroup.  ValueError where the library refuses nz."""
    nz = int(nz)
    tile = int(_capi.lib().drnmf_resample_tile(p, q, nz)) if -2 ** 31 <= nz < 2 ** 31 else 0
    if tile < 1:
        raise ValueError("resample: nz = %r is not a filter the kernel holds at p / q = %d / %d" % (nz, p, q))
    return int(_capi.lib().drnmf_resample_taps_len(p, q, nz)), tile


def resample_tile(fs_in, fs_out, nz=RESAMPLE_NZ):
    """The outputs one workgroup of the kernel owns at this rate (drnmf_resample_tile)."""
    return _resample_filter_shape(*resample_rate(fs_in, fs_out), nz=nz)[1]


_resample_taps_cache = {}


def resample_taps(p, q, nz=RESAMPLE_NZ, beta=RESAMPLE_BETA, device=None):
    """The filter of include/drnmf_resample.h for a reduced p / q, fp64 [L] on the device: computed there once per
    (device, p, q, nz, beta) and kept.  A later caller's stream waits for the launch that filled it."""
    di = _dev_of('cuda' if device is None else device)
    beta = float(beta)
    if not 0.0 <= beta < 1e3:
        raise ValueError("resample: beta = %r must lie in [0, 1000)" % beta)
    key = (di, int(p), int(q), int(nz), beta)
    if key not in _resample_taps_cache:
        L, _ = _resample_filter_shape(int(p), int(q), nz)
        with torch.cuda.device(di):
            taps = torch.empty(L, dtype=torch.float64, device=torch.device('cuda', di))
            _call("drnmf_resample_taps", di, int(p), int(q), int(nz), beta, _capi.ptr(taps))
            ev = torch.cuda.Event()
            ev.record()
        _resample_taps_cache[key] = (taps, ev)
    taps, ev = _resample_taps_cache[key]
    torch.cuda.current_stream(di).wait_event(ev)
    return taps


def _resample_input(x, lengths, dev, what):
    """(pcm [n][stride] on dev, host lengths int64 [n], device lengths or None) of what `resample` takes: a list of
    1-D arrays, or a 2-D array / device tensor with lengths=."""
    if isinstance(x, torch.Tensor) or (isinstance(x, np.ndarray) and x.ndim == 2):
        if lengths is None:
            raise ValueError("%s: a 2-D array or tensor comes with lengths=" % what)
        lens = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths, dtype=np.int64).reshape(-1)
        if isinstance(x, np.ndarray):
            if x.dtype not in (np.dtype('int16'), np.dtype('float32')):
                raise ValueError("%s: samples must be int16 or float32 (got %s)" % (what, x.dtype))
            x = _upload_pinned(x, dev)
        if x.dim() != 2 or x.dtype not in (torch.int16, torch.float32) or not x.is_contiguous() or x.shape[0] < 1 \
                or x.shape[1] < 1:
            raise ValueError("%s: samples must be a contiguous 2-D int16 or float32 tensor [n][stride] (got %s %s)"
                             % (what, x.dtype, tuple(x.shape)))
        if x.device != dev:
            raise ValueError("%s: the samples are on %s, the call on %s" % (what, x.device, dev))
        if lens.shape[0] != x.shape[0] or lens.min() < 0 or lens.max() > x.shape[1]:
            raise ValueError("%s: lengths must be %d values in [0, %d]" % ((what,) + tuple(x.shape)))
        return x, lens, None
    if lengths is not None:
        raise ValueError("%s: lengths= goes with a 2-D array, not with a list" % what)
    rows = [np.asarray(v) for v in x]
    if not rows:
        raise ValueError("%s: no waveforms" % what)
    dt = rows[0].dtype
    if dt not in (np.dtype('int16'), np.dtype('float32')):
        raise ValueError("%s: waveforms must be int16 or float32 (got %s)" % (what, dt))
    for v in rows:
        if v.ndim != 1 or v.dtype != dt:
            raise ValueError("%s: every waveform must be a 1-D %s array (one type per call)" % (what, dt))
    lens = np.array([v.shape[0] for v in rows], dtype=np.int64)
    if lens.max() < 1:          # nothing to upload; a row width of one keeps the strides positive
        tdt = torch.int16 if dt == np.dtype('int16') else torch.float32
        return torch.zeros((len(rows), 1), dtype=tdt, device=dev), lens, torch.zeros(len(rows), dtype=torch.int64,
                                                                                     device=dev)
    pcm, lens_d = _upload_wav_side(rows, dt, dev)
    return pcm, lens, lens_d


def resample(x, fs_in, fs_out, lengths=None, out=None, nz=RESAMPLE_NZ, beta=RESAMPLE_BETA, device=None):
    """Waveforms at fs_in converted to fs_out on the device (drnmf_resample_forward; the definition -- Matlab's
    `resample` filter with nz zero crossings a side and Kaiser beta, one ascending fp64 chain per output, rounded
    once to float32 -- is in include/drnmf_resample.h).  x: a list of 1-D int16 (scaled by 1/32768) or float32 numpy
    arrays of any lengths, 0 included, or a 2-D array / device tensor [n][stride] with lengths=.  Returns (y,
    out_lengths): float32 [n][max(1, max out_lengths)] on the device, zeros behind a row's length, and
    out_lengths = ceil(lengths p / q) int64 on the host.  out=: a float32 [n][width] tensor at least that wide, written
    whole and returned.  Equal rates copy (int16 converted).  Enqueues only; a list goes up in one pinned copy."""
    p, q = resample_rate(fs_in, fs_out)
    L, _ = _resample_filter_shape(p, q, nz)
    if isinstance(x, torch.Tensor):
        dev = torch.device('cuda', _dev_index(x))
    else:
        dev = torch.device('cuda', _dev_of('cuda' if device is None else device))
    with torch.cuda.device(dev):
        pcm, lens, lens_d = _resample_input(x, lengths, dev, "resample")
        n_out = -(-lens * p // q)
        n, need = pcm.shape[0], max(1, int(n_out.max()))
        if out is None:
            out = torch.empty((n, need), dtype=torch.float32, device=dev)
        elif not isinstance(out, torch.Tensor) or out.dim() != 2 or out.shape[0] != n or out.shape[1] < need or \
                out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise ValueError("resample: out must be a contiguous float32 tensor [%d][>= %d] on %s" % (n, need, dev))
        if lens_d is None:
            lens_d = _upload_pinned(lens, dev)
        taps = resample_taps(p, q, nz, beta, dev) if L else None
        _call("drnmf_resample_forward", _dev_index(pcm), n, pcm.shape[1], _capi.ptr(lens_d),
              int(pcm.dtype == torch.int16), _capi.ptr(pcm), p, q, int(nz), _capi.ptr(taps), out.shape[1],
              _capi.ptr(out))
    return out, n_out


def resample_wavs(x, fs_in, fs_out, lengths=None, nz=RESAMPLE_NZ, beta=RESAMPLE_BETA, device=None):
    """`resample` and the one download: a list of float32 numpy arrays, row i ceil(len_i p / q) samples."""
    y, n_out = resample(x, fs_in, fs_out, lengths=lengths, nz=nz, beta=beta, device=device)
    host = y.cpu().numpy()
    return [host[i, :int(k)].copy() for i, k in enumerate(n_out)]


class ResampleStream(object):
    """`resample` for audio that arrives piece by piece, n_streams recordings side by side.  push(chunks) takes one
    chunk per stream (1-D numpy arrays of the stream's dtype, 'float32' or 'int16'; any lengths, 0 included) and
    returns, per stream, the float32 outputs that have become final: output m is final once sample floor((q m +
    half) / p) has arrived.  close() returns the rest, reset() starts over.  Over all pushes a stream yields
    exactly ceil(n p / q) samples, with the bits of `resample` on the whole recording however it was cut: the same
    kernel sums the same chain (drnmf_resample_chunk).  The samples a later output still needs -- at most about
    (L - 1) / p + q / p + 1 a stream -- stay on the device (drnmf_resample_carry moves them to the front of the next
    row and appends the new chunk); the counters live on the host.  A push is one pinned upload, two launches and
    one download."""

    def __init__(self, n_streams, fs_in, fs_out, dtype='float32', device=None, nz=RESAMPLE_NZ, beta=RESAMPLE_BETA):
        if dtype not in ('int16', 'float32'):
            raise ValueError("ResampleStream: dtype must be 'int16' or 'float32'")
        if int(n_streams) < 1 or int(n_streams) > 65535:
            raise ValueError("ResampleStream: n_streams = %r must lie in [1, 65535]" % (n_streams,))
        self.n_streams, self.dtype = int(n_streams), np.dtype(dtype)
        self.p, self.q = resample_rate(fs_in, fs_out)
        self.nz = int(nz)
        L, _ = _resample_filter_shape(self.p, self.q, self.nz)
        self.L = L if L else 1                                  # the copy: a filter of one tap
        self.half = (self.L - 1) // 2
        self.device = torch.device('cuda', _dev_of('cuda' if device is None else device))
        self._taps = resample_taps(self.p, self.q, self.nz, beta, self.device) if L else None
        self.reset()

    def reset(self):
        """Every stream empty and open."""
        n = self.n_streams
        self.n_in = np.zeros(n, dtype=np.int64)         # samples arrived
        self.n_out = np.zeros(n, dtype=np.int64)        # outputs returned
        self.held_from = np.zeros(n, dtype=np.int64)    # the first sample the device row holds
        tdt = torch.int16 if self.dtype == np.dtype('int16') else torch.float32
        self._rows = [torch.empty((n, 1), dtype=tdt, device=self.device) for _ in range(2)]     # [0]: the history
        self.closed = False

    def _first_needed(self, m):
        lo = self.q * m + self.half - (self.L - 1)
        return np.maximum(-(-lo // self.p), 0)

    def push(self, chunks, final=False):
        if self.closed:
            raise ValueError("ResampleStream: the streams are closed; reset() starts over")
        rows = [np.asarray(c) for c in chunks]
        n, p, q = self.n_streams, self.p, self.q
        if len(rows) != n:
            raise ValueError("ResampleStream: %d chunks for %d streams" % (len(rows), n))
        for c in rows:
            if c.ndim != 1 or c.dtype != self.dtype:
                raise ValueError("ResampleStream: every chunk must be a 1-D %s array" % self.dtype)
        add = np.array([c.shape[0] for c in rows], dtype=np.int64)
        n_in = self.n_in + add
        if final:
            n_out = -(-n_in * p // q)
        else:
            n_out = np.maximum((p * n_in - 1 - self.half) // q + 1, self.n_out)
        # the row of this push: the history from the first sample that output self.n_out needs, then the chunk
        start = np.minimum(self._first_needed(self.n_out), self.n_in)
        drop, keep = start - self.held_from, self.n_in - start
        held, cnt = keep + add, n_out - self.n_out
        amax, width = int(add.max()), max(1, int(held.max()))
        prev, nxt = self._rows
        with torch.cuda.device(self.device):
            if nxt.shape[1] < width:
                nxt = torch.empty((n, -(-width // 1024) * 1024), dtype=prev.dtype, device=self.device)
            # one pinned upload: eight int64 tables [n] | the chunks [n][amax]
            isz = self.dtype.itemsize
            host = torch.empty(64 * n + n * amax * isz, dtype=torch.uint8, pin_memory=True)
            hn = host.numpy()
            tab = hn[:64 * n].view(np.int64).reshape(8, n)
            for r, v in enumerate((drop, keep, add, held, start, self.n_out, cnt,
                                   n_in if final else np.full(n, -1, dtype=np.int64))):
                tab[r] = v
            if amax:
                pk = hn[64 * n:].view(self.dtype).reshape(n, amax)
                for i, c in enumerate(rows):
                    pk[i, :c.shape[0]] = c
            d = host.to(self.device, non_blocking=True)
            t = d[:64 * n].view(torch.int64).view(8, n)
            chunk = d[64 * n:].view(prev.dtype).view(n, amax) if amax else None
            di = _dev_of(self.device)
            _call("drnmf_resample_carry", di, n, int(self.dtype == np.dtype('int16')), prev.shape[1], _capi.ptr(prev),
                  amax, _capi.ptr(chunk), _capi.ptr(t[0]), _capi.ptr(t[1]), _capi.ptr(t[2]), nxt.shape[1],
                  _capi.ptr(nxt))
            y = None
            if int(cnt.max()) > 0:
                y = torch.empty((n, int(cnt.max())), dtype=torch.float32, device=self.device)
                _call("drnmf_resample_chunk", di, n, nxt.shape[1], _capi.ptr(t[3]), _capi.ptr(t[4]), _capi.ptr(t[5]),
                      _capi.ptr(t[6]), _capi.ptr(t[7]), int(self.dtype == np.dtype('int16')), _capi.ptr(nxt), p, q,
                      self.nz, _capi.ptr(self._taps), y.shape[1], _capi.ptr(y))
            self._rows = [nxt, prev]
            self.n_in, self.n_out, self.held_from = n_in, n_out, start
            self.closed = bool(final)
            if y is None:
                return [np.zeros(0, dtype=np.float32) for _ in range(n)]
            yh = y.cpu().numpy()
        return [yh[i, :int(k)].copy() for i, k in enumerate(cnt)]

    def close(self):
        """End every stream: the outputs still held back, cut at ceil(n p / q)."""
        return self.push([np.zeros(0, dtype=self.dtype) for _ in range(self.n_streams)], final=True)


# ---- mixtures of a speech bank and a noise bank on the device (include/drnmf_mix.h) -------------------------
def _mix_pcm(t, name):
    if t.dim() != 2 or t.dtype not in (torch.int16, torch.float32) or not t.is_contiguous() or t.shape[0] < 1 \
            or t.shape[1] < 1:
        raise ValueError("%s must be a contiguous 2-D int16 or float32 tensor [n][stride] (got %s %s)"
                         % (name, t.dtype, tuple(t.shape)))
    return t


def _mix_table(t, n, dtype, name):
    if t.dtype != dtype or t.dim() != 1 or t.shape[0] != n or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s tensor [%d] (got %s %s)" % (name, dtype, n, t.dtype,
                                                                                 tuple(t.shape)))
    return t


def mix_workspace(n_sig, stride, device, have=None):
    """The workspace of mix_energy / mix_forward for n_sig signals of `stride` samples (`have`: kept if it is
    large enough)."""
    return _workspace(int(_capi.lib().drnmf_mix_workspace_bytes(int(n_sig), int(stride))), device, have)


def mix_energy(pcm, lengths, out=None, workspace=None):
    """drnmf_mix_energy: the fp64 sum of squares of every row of pcm [n][stride] (int16, scaled by 1/32768, or
    float32) over its own length (int64 [n] on the device), in the fixed order of include/drnmf_mix.h.  Enqueues
    only."""
    _mix_pcm(pcm, "pcm")
    n, stride = pcm.shape
    _mix_table(lengths, n, torch.int64, "lengths")
    dev = _dev_index(pcm)
    out = _out(out, (n,), torch.float64, pcm.device)
    ws = mix_workspace(n, stride, pcm.device, workspace)
    _call("drnmf_mix_energy", dev, n, stride, _capi.ptr(lengths), int(pcm.dtype == torch.int16), _capi.ptr(pcm),
          _capi.ptr(out), _capi.ptr(ws), ws.numel())
    return out


def mix_forward(speech, len_s, noise, len_n, noise_index, offset, snr_db, speech_energy=None, out=None,
                workspace=None, return_gain=False):
    """drnmf_mix_forward: noisy[i] = speech[i] + g_i * (noise[noise_index[i]] read from offset[i], wrapped), with
    g_i the gain that realises snr_db[i] over the whole signal (no speech-activity weighting); see
    include/drnmf_mix.h for the definition, the degenerate rows (g = 0) and the order of the sums.  speech
    [n][stride_s] and noise [m][stride_n] int16 or float32 (independently), len_s / len_n int64, noise_index int32,
    offset int64, snr_db float32, all on the device.  speech_energy: mix_energy(speech, len_s) if the caller keeps
    it.  Returns noisy float32 [n][stride_s] (`out` if given), and the gains [n] with return_gain.  Enqueues
    only."""
    _mix_pcm(speech, "speech")
    _mix_pcm(noise, "noise")
    n, stride_s = speech.shape
    m, stride_n = noise.shape
    _mix_table(len_s, n, torch.int64, "len_s")
    _mix_table(len_n, m, torch.int64, "len_n")
    _mix_table(noise_index, n, torch.int32, "noise_index")
    _mix_table(offset, n, torch.int64, "offset")
    _mix_table(snr_db, n, torch.float32, "snr_db")
    if speech_energy is not None:
        _mix_table(speech_energy, n, torch.float64, "speech_energy")
    dev = speech.device
    out = _out(out, (n, stride_s), torch.float32, dev)
    for t in (len_s, noise, len_n, noise_index, offset, snr_db, speech_energy):
        if t is not None and t.device != dev:
            raise ValueError("mix_forward: every tensor must be on %s" % dev)
    gain = torch.empty(n, dtype=torch.float32, device=dev) if return_gain else None
    di = _dev_index(speech)
    ws = mix_workspace(n, stride_s, dev, workspace)
    _call("drnmf_mix_forward", di, n, stride_s, _capi.ptr(len_s), int(speech.dtype == torch.int16),
          _capi.ptr(speech), m, stride_n, _capi.ptr(len_n), int(noise.dtype == torch.int16), _capi.ptr(noise),
          _capi.ptr(noise_index), _capi.ptr(offset), _capi.ptr(snr_db), _capi.ptr(speech_energy), _capi.ptr(out),
          _capi.ptr(gain), _capi.ptr(ws), ws.numel())
    return (out, gain) if return_gain else out


# ---- reverberation of a speech bank on the device (include/drnmf_reverb.h) ----------------------------------
REVERB_TILE, REVERB_CHUNK = _capi.REVERB_TILE, _capi.REVERB_CHUNK
TARGET_SPEECH = ('reverberant', 'early', 'dry')


def reverb_forward(speech, len_s, rirs, len_r, rir_index, delay=None, n_early=None, out=None, early_out=None,
                   return_early=False):
    """drnmf_reverb_forward: wet[i] = speech[i] convolved with rirs[rir_index[i]], moved forward by that RIR's
    delay so that it stays aligned with the dry speech, and cut to the signal's length; early[i] the same sum over
    the RIR's first n_early taps only.  See include/drnmf_reverb.h for the definition (one ascending fmaf chain
    per output and part) and the rows that stay dry (an index outside the bank, an empty RIR).  speech
    [n][stride_s] int16 or float32, rirs float32 [m][stride_r], len_s / len_r int64, rir_index int32 [n], delay /
    n_early int32 [m] or None (0 / all taps), all on the device.  Returns wet float32 [n][stride_s] (`out` if
    given), and early (`early_out` if given) with return_early or early_out.  Enqueues only."""
    _mix_pcm(speech, "speech")
    if rirs.dim() != 2 or rirs.dtype != torch.float32 or not rirs.is_contiguous() or rirs.shape[0] < 1 \
            or rirs.shape[1] < 1:
        raise ValueError("rirs must be a contiguous 2-D float32 tensor [n_rir][stride] (got %s %s)"
                         % (rirs.dtype, tuple(rirs.shape)))
    n, stride_s = speech.shape
    m, stride_r = rirs.shape
    _mix_table(len_s, n, torch.int64, "len_s")
    _mix_table(len_r, m, torch.int64, "len_r")
    _mix_table(rir_index, n, torch.int32, "rir_index")
    if delay is not None:
        _mix_table(delay, m, torch.int32, "delay")
    if n_early is not None:
        _mix_table(n_early, m, torch.int32, "n_early")
    dev = speech.device
    out = _out(out, (n, stride_s), torch.float32, dev)
    want_early = return_early or early_out is not None
    early = _out(early_out, (n, stride_s), torch.float32, dev, "early_out") if want_early else None
    for t in (len_s, rirs, len_r, rir_index, delay, n_early):
        if t is not None and t.device != dev:
            raise ValueError("reverb_forward: every tensor must be on %s" % dev)
    _call("drnmf_reverb_forward", _dev_index(speech), n, stride_s, _capi.ptr(len_s), int(speech.dtype == torch.int16),
          _capi.ptr(speech), m, stride_r, _capi.ptr(len_r), _capi.ptr(rirs), _capi.ptr(rir_index), _capi.ptr(delay),
          _capi.ptr(n_early), _capi.ptr(out), _capi.ptr(early))
    return (out, early) if want_early else out


def _check_rirs(rirs, what):
    """Host-side checks of a bank of RIRs: a non-empty list of non-empty 1-D finite float32 arrays."""
    rows = [np.asarray(v) for v in rirs]
    if not rows:
        raise ValueError("%s: no RIRs" % what)
    for v in rows:
        if v.ndim != 1 or v.dtype != np.dtype('float32') or v.shape[0] < 1 or not np.isfinite(v).all():
            raise ValueError("%s: every RIR must be a non-empty 1-D finite float32 array" % what)
    return rows


def _check_reverb(rirs, align, target_speech, early_ms, fs, what):
    """What a bank with RIRs refuses before anything is uploaded.  Returns the RIR rows (None without RIRs)."""
    if target_speech not in TARGET_SPEECH:
        raise ValueError("%s: target_speech must be 'reverberant', 'early' or 'dry' (got %r)" % (what, target_speech))
    if not (np.isfinite(early_ms) and early_ms >= 0 and np.isfinite(fs) and fs > 0):
        raise ValueError("%s: early_ms = %r must be finite and >= 0, fs = %r positive" % (what, early_ms, fs))
    if rirs is None:
        return None
    rows = _check_rirs(rirs, what)
    if target_speech == 'dry' and not align:
        raise ValueError("%s: target_speech='dry' needs align=True (the dry target would lag the mixture by the "
                         "RIR's direct-path delay)" % what)
    return rows


def _check_side_rates(fs, clean_fs, noise_fs, rir_fs, rirs, what):
    """The three side rates of a bank against its fs, before anything is uploaded: each None where the side is
    taken as it is (not given, equal to fs, or rir_fs without RIRs), else a rate `resample` converts to fs."""
    out = []
    for side_fs, used in ((clean_fs, True), (noise_fs, True), (rir_fs, rirs is not None)):
        if side_fs is not None:
            try:
                p, q = resample_rate(side_fs, fs)
            except ValueError as e:
                raise ValueError("%s: %s" % (what, e))
            if (p, q) == (1, 1) or not used:
                side_fs = None
        out.append(side_fs)
    return out


def rir_delays(rirs):
    """The index of the first maximum of |h| of every RIR of a list (its direct-path tap), int32 [n_rir], on the
    host."""
    return np.array([int(np.argmax(np.abs(np.asarray(v)))) for v in _check_rirs(rirs, "rir_delays")], dtype=np.int32)


def rir_early_counts(delay, early_ms=50.0, fs=16000):
    """The early tap counts of RIRs whose direct-path taps are `delay`: delay + 1 + round(early_ms fs / 1000), int32,
    capped at 2^31 - 1 (the kernel clamps a count to the RIR's length, so any early_ms >= 0 is served).  On the
    host."""
    span = float(early_ms) * float(fs) / 1000.0
    if not (span >= 0.0):
        raise ValueError("rir_early_counts: early_ms = %r and fs = %r must give a span >= 0" % (early_ms, fs))
    top = 2 ** 31 - 1
    span = top if span >= top else int(round(span))            # before the add: the sum stays far inside an int64
    return np.minimum(np.asarray(delay, dtype=np.int64) + 1 + span, top).astype(np.int32)


def rir_draw(n, n_rir, seed=0, epoch=0, reverb_prob=1.0):
    """One epoch's RIR table for n signals over n_rir RIRs, on the host and a pure function of its arguments: int32
    [n], -1 where the utterance stays dry.  With rs = np.random.RandomState((seed * 998244353 + epoch * 7919 +
    0x52495221) % 2**32), a generator of its own (mix_draw's tables do not move when RIRs are added): idx =
    rs.randint(0, n_rir, n), then idx[rs.random_sample(n) >= reverb_prob] = -1."""
    reverb_prob = float(reverb_prob)
    if int(n) < 1 or int(n_rir) < 1 or not 0.0 <= reverb_prob <= 1.0:
        raise ValueError("rir_draw: n = %r signals, n_rir = %r RIRs (both positive) and reverb_prob = %r in [0, 1] "
                         "are needed" % (n, n_rir, reverb_prob))
    n = int(n)
    rs = np.random.RandomState((int(seed) * 998244353 + int(epoch) * 7919 + 0x52495221) % 2 ** 32)
    idx = rs.randint(0, int(n_rir), n).astype(np.int32)
    idx[rs.random_sample(n) >= reverb_prob] = -1
    return idx


SYNTHETIC_RIR_TAIL = 0.05       # standard deviation of synthetic_rirs' tail at the direct-path tap


def synthetic_rirs(n, fs=16000, rt60=(0.2, 0.8), seed=0):
    """n stand-in RIRs as float32 arrays, on the host: h[0] = 1 (the direct path), then white Gaussian noise of
    standard deviation SYNTHETIC_RIR_TAIL under an exponential envelope 10^(-3 t / (rt60 fs)), which reaches -60 dB
    at t = rt60 fs, the last tap; rt60 uniform in (lo, hi) seconds per RIR.  Reproducible from `seed`.  A stand-in
    with the length and decay of a room's response for tests and for users without measured RIRs -- not room
    acoustics: no early reflections, no frequency-dependent decay, no geometry."""
    lo, hi = float(rt60[0]), float(rt60[1])
    if int(n) < 1 or not (fs > 0 and 0 < lo <= hi and np.isfinite(hi)):
        raise ValueError("synthetic_rirs: n = %r, fs = %r and rt60 = (%r, %r) with 0 < lo <= hi are needed"
                         % (n, fs, lo, hi))
    rs = np.random.RandomState((int(seed) * 69069 + 0x53594e52) % 2 ** 32)
    out = []
    for _ in range(int(n)):
        taps = max(1, int(round((lo + (hi - lo) * rs.random_sample()) * fs)))
        t = np.arange(taps, dtype=np.float64)
        h = SYNTHETIC_RIR_TAIL * rs.standard_normal(taps) * 10.0 ** (-3.0 * t / taps)
        h[0] = 1.0
        out.append(h.astype(np.float32))
    return out


MIX_SNR_DB = (-6.0, 9.0)      # the SNR range of a draw that names neither snr_db nor snr_choices (CHiME2's)


def _check_mix_snr(snr_db, snr_choices, what):
    """(lo, hi, None) or (None, None, choices float32) of a draw, before anything else happens."""
    if snr_db is not None and snr_choices is not None:
        raise ValueError("%s: give snr_db=(lo, hi) or snr_choices=[...], not both" % what)
    if snr_choices is not None:
        c = np.asarray(snr_choices, dtype=np.float32)
        if c.ndim != 1 or c.size < 1 or not np.isfinite(c).all():
            raise ValueError("%s: snr_choices must be a non-empty list of finite values" % what)
        return None, None, c
    lo, hi = MIX_SNR_DB if snr_db is None else snr_db
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi:
        raise ValueError("%s: snr_db = (%r, %r) must be finite with lo <= hi" % (what, lo, hi))
    return lo, hi, None


def mix_draw(n, len_noise, snr_db=None, snr_choices=None, seed=0, epoch=0):
    """One epoch's mixing tables for n signals over noise recordings of len_noise samples, on the host and a pure
    function of its arguments: (noise_index int32 [n], offset int64 [n], snr float32 [n]).  With
    rs = np.random.RandomState((seed * 1000003 + epoch) % 2**32): noise_index = rs.randint(0, n_noise, n); offset
    = min(floor(rs.random_sample(n) * len_noise[noise_index]), len - 1); snr = lo + (hi - lo) * rs.random_sample(n)
    for snr_db=(lo, hi) (default MIX_SNR_DB) or choices[rs.randint(0, len(choices), n)] for snr_choices.  Giving
    both raises ValueError."""
    lo, hi, choices = _check_mix_snr(snr_db, snr_choices, "mix_draw")
    len_noise = np.asarray(len_noise, dtype=np.int64)
    if int(n) < 1 or len_noise.ndim != 1 or len_noise.size < 1 or (len_noise < 1).any():
        raise ValueError("mix_draw: n = %r signals and %d noise lengths, every one positive, are needed"
                         % (n, len_noise.size))
    n = int(n)
    rs = np.random.RandomState((int(seed) * 1000003 + int(epoch)) % 2 ** 32)
    idx = rs.randint(0, len_noise.size, n).astype(np.int32)
    ln = len_noise[idx]
    off = np.minimum(np.floor(rs.random_sample(n) * ln).astype(np.int64), ln - 1)
    if choices is None:
        snr = (lo + (hi - lo) * rs.random_sample(n)).astype(np.float32)
    else:
        snr = choices[rs.randint(0, choices.size, n)]
    return idx, off, snr


def _check_wav_side(rows, what, side):
    """Host-side checks of one side of a bank: a non-empty list of non-empty 1-D arrays of ONE type, int16 or
    float32.  Returns (rows, numpy dtype)."""
    rows = [np.asarray(v) for v in rows]
    if not rows:
        raise ValueError("%s: no %s waveforms" % (what, side))
    dt = rows[0].dtype
    if dt not in (np.dtype('int16'), np.dtype('float32')):
        raise ValueError("%s: %s waveforms must be int16 or float32 (got %s)" % (what, side, dt))
    for v in rows:
        if v.ndim != 1 or v.dtype != dt or v.shape[0] < 1:
            raise ValueError("%s: every %s waveform must be a non-empty 1-D %s array" % (what, side, dt))
    return rows, dt


class MixBank(object):
    """Clean speech and noise recordings, uploaded once, from which every epoch's noisy training data is mixed on
    the device: noisy = speech + g * noise at a drawn SNR (mix_forward), then the pair kernels of
    wavs_to_tensors on (noisy, clean).  A new draw costs three small index tables and two passes over samples
    already in device memory; the clean side decides the frame counts, so the shapes of (x, y, w) are the same
    for every draw and a draw can be rewritten into the same tensors (out=).

    clean, noise: lists of 1-D int16 or float32 arrays, one type per side (the sides may differ).  The clean
    side is kept as float32 (int16 converted once, v / 32768: the pair kernels take both members of a pair in one
    type), the noise side in the type it came in.  SNRs are over the whole utterance (no speech-activity
    weighting); mixtures are not clipped and may exceed +-1.

    rirs: a list of non-empty 1-D finite float32 arrays puts the speech in a room first (reverb_forward, include/
    drnmf_reverb.h): noisy = wet + g * noise with wet the clean utterance convolved with the RIR a draw names for
    it (a draw is then a 4-tuple, its last table the RIR per utterance, -1: the utterance stays dry), and the SNR
    is that of the REVERBERANT speech in the mixture.  The RIRs, their lengths, delays and early counts go up
    once.  align=True moves every wet signal forward by its RIR's direct-path delay (rir_delays), so that it stays
    aligned with the dry speech; align=False is the causal convolution cut to the utterance's length.
    target_speech: what the pair kernels get as the clean member -- 'reverberant' (wet: the CHiME2 convention, the
    model removes noise only), 'early' (the direct path and the reflections up to early_ms after it: the model
    also removes late reverberation) or 'dry' (the bank's clean side; needs align=True).  rirs=None: the bank of
    before, the same launches and the same bits.

    clean_fs, noise_fs, rir_fs: the rate a side comes at.  A side whose rate is given and differs from fs is
    resampled to fs once, on the device, while the bank is built (`resample`, include/drnmf_resample.h), and is
    then held as float32; everything after that -- lengths, the energy table, draws, tensors, frames, wavs -- is the
    bank built from resample_wavs(side, side_fs, fs).  An RIR is resampled like any waveform: its samples follow the
    definition, so its gain as a filter scales by fs / rir_fs (the SNR of a mixture is that of the wet speech either
    way).  None (and a rate equal to fs): the side is taken as it is, the same launches and bits as before."""

    def __init__(self, clean, noise, rirs=None, align=True, target_speech='reverberant', early_ms=50.0, fs=16000,
                 device=None, clean_fs=None, noise_fs=None, rir_fs=None):
        ry, dty = _check_wav_side(clean, "MixBank", "clean")
        rn, dtn = _check_wav_side(noise, "MixBank", "noise")
        rr = _check_reverb(rirs, align, target_speech, early_ms, fs, "MixBank")
        clean_fs, noise_fs, rir_fs = _check_side_rates(fs, clean_fs, noise_fs, rir_fs, rirs, "MixBank")
        self.target_speech, self.n_rir = target_speech, (0 if rr is None else len(rr))
        if dty == np.dtype('int16') and clean_fs is None:
            ry = [v.astype(np.float32) / np.float32(32768.0) for v in ry]
        self.n, self.n_noise = len(ry), len(rn)
        dev = torch.device('cuda' if device is None else device)
        self.device = torch.device('cuda', _dev_of(dev))

        def side(rows, dt, side_fs):
            """(samples, lengths on the device, lengths on the host) of one side at fs"""
            if side_fs is None:
                return _upload_wav_side(rows, dt, self.device) + (np.array([v.shape[0] for v in rows], dtype=np.int64),)
            y, n_out = resample(rows, side_fs, fs, device=self.device)
            return y, _upload_pinned(n_out, self.device), n_out
        with torch.cuda.device(self.device):
            self.clean, self.len_clean_dev, self.len_clean = side(ry, np.dtype('float32') if clean_fs is None else dty,
                                                                  clean_fs)
            self.noise, self.len_noise_dev, self.len_noise = side(rn, dtn, noise_fs)
            self.workspace = mix_workspace(self.n, self.clean.shape[1], self.device)
            # (a bank with RIRs mixes the wet speech, whose energy changes with the draw: mix_forward computes it)
            self.energy = None if rr is not None else mix_energy(self.clean, self.len_clean_dev,
                                                                 workspace=self.workspace)
            self.noisy = torch.empty(tuple(self.clean.shape), dtype=torch.float32, device=self.device)
            if rr is not None:
                self.rirs, self.len_rir_dev, len_rir = side(rr, np.dtype('float32'), rir_fs)
                if rir_fs is not None and align:        # the direct-path taps are those of the RIRs at fs
                    host = self.rirs.cpu().numpy()
                    rr = [host[i, :int(k)] for i, k in enumerate(len_rir)]
                delay = rir_delays(rr) if align else np.zeros(len(rr), dtype=np.int32)
                taps = np.stack([delay, rir_early_counts(delay, early_ms, fs)])
                taps_d = _upload_pinned(taps, self.device)
                self.rir_delay, self.rir_n_early = taps_d[0], taps_d[1]
                self.wet = torch.empty_like(self.noisy)
                self.early = torch.empty_like(self.noisy) if target_speech == 'early' else None
        self._tables = {}

    def draw(self, snr_db=None, snr_choices=None, seed=0, epoch=0, reverb_prob=1.0):
        """mix_draw for this bank: (noise_index, offset, snr) on the host, a pure function of the arguments.  A
        bank with RIRs appends rir_draw's table: (noise_index, offset, snr, rir_index), the first three as
        without RIRs; reverb_prob: the probability that an utterance is reverberated."""
        d = mix_draw(self.n, self.len_noise, snr_db=snr_db, snr_choices=snr_choices, seed=seed, epoch=epoch)
        if not self.n_rir:
            return d
        return d + (rir_draw(self.n, self.n_rir, seed=seed, epoch=epoch, reverb_prob=reverb_prob),)

    def _check_draw(self, draw):
        what = "(noise_index, offset, snr, rir_index)" if self.n_rir else "(noise_index, offset, snr)"
        try:
            if self.n_rir:
                idx, off, snr, ridx = draw
            else:
                (idx, off, snr), ridx = draw, None
        except (TypeError, ValueError):
            raise ValueError("MixBank: a draw is %s" % what)
        idx, off, snr = np.asarray(idx), np.asarray(off), np.asarray(snr)
        tables = [(idx, np.int32, "noise_index"), (off, np.int64, "offset"), (snr, np.float32, "snr")]
        if self.n_rir:
            ridx = np.asarray(ridx)
            tables.append((ridx, np.int32, "rir_index"))
        for a, dt, name in tables:
            if a.dtype != np.dtype(dt) or a.shape != (self.n,):
                raise ValueError("MixBank: %s must be %s [%d] (got %s %s)" % (name, np.dtype(dt), self.n, a.dtype,
                                                                              a.shape))
        if idx.min() < 0 or idx.max() >= self.n_noise:
            raise ValueError("MixBank: noise_index outside [0, %d)" % self.n_noise)
        if self.n_rir and (ridx.min() < -1 or ridx.max() >= self.n_rir):
            raise ValueError("MixBank: rir_index outside [-1, %d)" % self.n_rir)
        return (idx, off, snr, ridx) if self.n_rir else (idx, off, snr)

    def _mix_reverberant(self, draw):
        """mix() of a bank with RIRs: wet (and early) from the clean side, then the mixer on wet."""
        idx, off, snr, ridx = draw
        with torch.cuda.device(self.device):
            # one pinned upload: offset [n] int64 | noise_index [n] int32 | snr [n] float32 | rir_index [n] int32
            n = self.n
            host = torch.empty(20 * n, dtype=torch.uint8, pin_memory=True)
            hn = host.numpy()
            hn[:8 * n].view(np.int64)[:] = off
            hn[8 * n:12 * n].view(np.int32)[:] = idx
            hn[12 * n:16 * n].view(np.float32)[:] = snr
            hn[16 * n:].view(np.int32)[:] = ridx
            d = host.to(self.device, non_blocking=True)
            reverb_forward(self.clean, self.len_clean_dev, self.rirs, self.len_rir_dev, d[16 * n:].view(torch.int32),
                           delay=self.rir_delay, n_early=self.rir_n_early, out=self.wet, early_out=self.early)
            # the speech energy is the wet signal's, computed by the call: the SNR is the reverberant speech's
            mix_forward(self.wet, self.len_clean_dev, self.noise, self.len_noise_dev, d[8 * n:12 * n].view(torch.int32),
                        d[:8 * n].view(torch.int64), d[12 * n:16 * n].view(torch.float32), speech_energy=None,
                        out=self.noisy, workspace=self.workspace)
        return self.noisy, self.len_clean_dev

    def _target(self):
        """The clean member of the pairs: what target_speech names (valid after mix() for 'reverberant' and
        'early')."""
        if not self.n_rir or self.target_speech == 'dry':
            return self.clean
        return self.wet if self.target_speech == 'reverberant' else self.early

    def mix(self, draw):
        """(noisy float32 [n][stride], lengths int64 [n]) on the device.  noisy is the bank's own buffer: the next
        mix overwrites it (and, with RIRs, the wet and early buffers beside it)."""
        if self.n_rir:
            return self._mix_reverberant(self._check_draw(draw))
        idx, off, snr = self._check_draw(draw)
        with torch.cuda.device(self.device):
            # one pinned upload: offset [n] int64 | noise_index [n] int32 | snr [n] float32
            n = self.n
            host = torch.empty(16 * n, dtype=torch.uint8, pin_memory=True)
            hn = host.numpy()
            hn[:8 * n].view(np.int64)[:] = off
            hn[8 * n:12 * n].view(np.int32)[:] = idx
            hn[12 * n:].view(np.float32)[:] = snr
            d = host.to(self.device, non_blocking=True)
            mix_forward(self.clean, self.len_clean_dev, self.noise, self.len_noise_dev, d[8 * n:12 * n].view(torch.int32),
                        d[:8 * n].view(torch.int64), d[12 * n:].view(torch.float32), speech_energy=self.energy,
                        out=self.noisy, workspace=self.workspace)
        return self.noisy, self.len_clean_dev

    def _frame_counts(self, N, hop, transform, what):
        N, hop = int(N), int(hop)
        if transform not in _capi.TRANSFORMS:
            raise ValueError("%s: transform must be 'mag' or 'logmag' (got %r)" % (what, transform))
        if N < 64 or N > 4096 or N & (N - 1) or hop < 1:
            raise ValueError("%s: N = %d must be a power of two in [64, 4096] and hop = %d positive" % (what, N, hop))
        return -(-self.len_clean // hop) + N // hop + 1               # drnmf_stft_frames

    def _table(self, kind, N, hop, maxlen, build):
        key = (kind, int(N), int(hop), maxlen)
        if key not in self._tables:
            self._tables[key] = build()
        return self._tables[key]

    def tensors(self, draw, N=512, hop=128, maxlen=None, transform='mag', mask_value=None, target='mag', out=None):
        """(x, y, w) of one draw, exactly what wavs_to_tensors(self.wavs(draw), clean as float32, ...) returns, by
        the same launches on (noisy, clean) without the download and the two uploads (with RIRs: clean is
        self.target_wavs(draw), the side target_speech names).  The sequence table is
        uploaded once per (N, hop, maxlen).  out=(x, y, w): tensors of an earlier call with the same arguments,
        rewritten in place and returned.  Enqueues only."""
        from . import data
        _check_target(target, transform, "MixBank.tensors")
        nf = self._frame_counts(N, hop, transform, "MixBank.tensors")
        self._check_draw(draw)

        def build():
            table, T = data.sequence_table_from_lengths(nf, maxlen)
            return _upload_pinned(table, self.device), T
        with torch.cuda.device(self.device):
            table_d, T = self._table('seq', N, hop, maxlen, build)
            if mask_value is None:
                mask_value = data.get_mask_value(dict(transform_x=transform, transform_y=transform))
            n_seq, F = table_d.shape[0], int(N) // 2 + 1
            x, y, w = (None, None, None) if out is None else out
            x = _out(x, (n_seq, T, F), torch.float32, self.device, "MixBank.tensors: out[0] (x)")
            y = _out(y, (n_seq, T, F), torch.float32, self.device, "MixBank.tensors: out[1] (y)")
            w = _out(w, (n_seq, T), torch.float32, self.device, "MixBank.tensors: out[2] (w)")
            noisy, ln = self.mix(draw)
            if target == 'mag':
                stft_pair_chunks_enqueue(noisy, self._target(), ln, ln, table_d, T, N, hop, transform, mask_value, x, y,
                                         w)
            else:
                stft_pair_target_enqueue(noisy, self._target(), ln, ln, table_d, T, N, hop, transform, target,
                                         mask_value, x, y, w)
        return x, y, w

    def frames(self, draw, N, hop, transform='mag'):
        """(x_frames, y_frames) of one draw: the packed rows wavs_to_frames gives for (self.wavs(draw), clean)."""
        nf = self._frame_counts(N, hop, transform, "MixBank.frames")
        self._check_draw(draw)
        with torch.cuda.device(self.device):
            row0 = self._table('row0', N, hop, None, lambda: _upload_pinned(np.cumsum(nf) - nf, self.device))
            xf = torch.empty((int(nf.sum()), int(N) // 2 + 1), dtype=torch.float32, device=self.device)
            yf = torch.empty_like(xf)
            noisy, ln = self.mix(draw)
            stft_pair_frames_enqueue(noisy, self._target(), ln, ln, row0, N, hop, transform, xf, yf)
        return xf, yf

    def _download(self, pcm):
        host = pcm.cpu().numpy()
        return [host[i, :int(k)].copy() for i, k in enumerate(self.len_clean)]

    def wavs(self, draw):
        """The mixtures of one draw as a list of float32 numpy arrays: the one call that downloads (a fixed
        validation set, listening)."""
        return self._download(self.mix(draw)[0])

    def clean_wavs(self):
        """The clean side as the bank holds it: a list of float32 numpy arrays (downloads)."""
        return self._download(self.clean)

    def target_wavs(self, draw):
        """The target side of one draw, what `tensors` and `frames` pair the mixtures with: the wet speech, its
        early part or the clean side as target_speech says (the clean side without RIRs), as a list of float32
        numpy arrays (downloads)."""
        self.mix(draw)
        return self._download(self._target())


def istft_ragged_enqueue(re, im, mask, lengths_dev, sig_index_dev, N, hop, y, crop, workspace=None):
    """drnmf_istft_ragged on tensors the caller owns and has checked: enqueues, reads nothing back."""
    dev = _dev_index(re)
    b, T, F = re.shape
    nbytes = _capi.lib().drnmf_istft_ragged_workspace_bytes(b, T, int(N), int(hop))
    if nbytes:                      # (0: the entry needs none, and takes the caller's, or NULL, as it is)
        workspace = _workspace(nbytes, re.device, workspace)
    _call("drnmf_istft_ragged", dev, y.shape[0], b, T, int(N), int(hop), _capi.ptr(lengths_dev),
          _capi.ptr(sig_index_dev), _capi.ptr(re), _capi.ptr(im), _capi.ptr(mask),
          0 if mask is None else mask.stride(1), _capi.ptr(y), y.shape[1], int(bool(crop)), _capi.ptr(workspace),
          0 if workspace is None else workspace.numel())


def istft_ragged(re, im, mask, lengths, N, hop, sig_index=None, out=None, crop=False):
    """Masked inverse of a slab: y[sig_index[k], :n_k] = istft_noDiv(mask[k] * (re[k] + i im[k])) (`istft_masked`
    per row), zeros behind n_k = ragged_out_lengths(lengths, N, hop, crop)[sig_index[k]].  re, im, mask [b, T,
    N/2+1] device float32 (mask may be None, or the model's output with a padded last stride); lengths [n_sig]
    host ints or a tensor; out [n_sig, width] float32 (default: zeros of the widest row).  Rows of `out` that
    sig_index does not name are left as they are.  A row's samples are bitwise the same in any batch."""
    if re.dim() != 3 or re.shape != im.shape or re.shape[2] != N // 2 + 1:
        raise ValueError("istft_ragged: re, im must be [b, T, %d] (got %s, %s)" % (N // 2 + 1, tuple(re.shape),
                                                                                  tuple(im.shape)))
    dev = re.device
    _dev_index(re)
    re, im = _f32c(re, "re"), _f32c(im, "im")
    if im.device != dev:
        raise ValueError("istft_ragged: re and im must be on one device")
    b, T, F = re.shape
    if mask is not None:
        if mask.dtype != torch.float32 or mask.device != dev or tuple(mask.shape) != (b, T, F):
            raise ValueError("istft_ragged: mask must be float32 %s on %s" % ((b, T, F), dev))
        if mask.stride(2) != 1 or mask.stride(1) < F or mask.stride(0) != T * mask.stride(1):
            mask = mask.contiguous()
    if int(hop) < 1:
        raise ValueError("istft_ragged: hop < 1")
    if out is not None:
        # any [n_sig, width] is taken: (-1, -1) stands for that in the message, and matches no other rank
        _given(out, tuple(out.shape) if out.dim() == 2 else (-1, -1), torch.float32, dev, "istft_ragged: out")
        n_sig = out.shape[0]
    else:
        n_sig = lengths.numel() if isinstance(lengths, torch.Tensor) else np.asarray(lengths).size
    lh, ld = _ragged_lengths(lengths, n_sig, 1 << 40, dev, "istft_ragged")
    idx = _ragged_index(sig_index, n_sig, dev, "istft_ragged")
    if idx.numel() != b:
        raise ValueError("istft_ragged: %d slab rows but sig_index names %d" % (b, idx.numel()))
    if out is None:
        out = torch.zeros((n_sig, max(1, int(ragged_out_lengths(lh, N, hop, crop).max()))), dtype=torch.float32,
                          device=dev)
    istft_ragged_enqueue(re, im, mask, ld, idx, N, hop, out, crop)
    return out


def to_int16_wav_rows_enqueue(y, lengths_dev, out, workspace=None):
    dev = _dev_index(y)
    n_sig, stride = y.shape
    workspace = _workspace(_capi.lib().drnmf_wav_int16_rows_workspace_bytes(n_sig), y.device, workspace)
    _call("drnmf_wav_int16_rows", dev, n_sig, stride, _capi.ptr(lengths_dev), _capi.ptr(y), _capi.ptr(out),
          _capi.ptr(workspace), workspace.numel())


def to_int16_wav_rows(y, lengths):
    """`to_int16_wav` per row (util.wavwrite, util.py:37-45, one file per row): y [n_sig, stride] float32, row k
    valid up to lengths[k]; row k of the int16 result equals to_int16_wav(y[k, :lengths[k]]) and is 0 behind it."""
    if y.dim() != 2:
        raise ValueError("to_int16_wav_rows: y must be [n_sig, stride]")
    _dev_index(y)
    y = _f32c(y, "y")
    n_sig, stride = y.shape
    if n_sig < 1 or stride < 1:
        raise ValueError("to_int16_wav_rows: empty batch")
    _, ld = _ragged_lengths(lengths, n_sig, stride, y.device, "to_int16_wav_rows")
    out = torch.empty((n_sig, stride), dtype=torch.int16, device=y.device)
    to_int16_wav_rows_enqueue(y, ld, out)
    return out


# ---- streaming: chunks in, finished samples out (include/drnmf_stream.h) --------------------------------------
def stream_counts(n_samples, closed, N, hop, crop=False):
    """(frames, samples) a stream holds after n_samples samples, open or closed (drnmf_stream_counts).  A stream
    that has never been pushed has (0, 0)."""
    L = _capi.lib()
    f, s = _capi.C.c_int64(), _capi.C.c_int64()
    rc = L.drnmf_stream_counts(int(n_samples), int(bool(closed)), int(N), int(hop), int(bool(crop)),
                               _capi.C.byref(f), _capi.C.byref(s))
    if rc != _capi.OK:
        raise ValueError("stream_counts: n_samples = %d must not be negative and hop = %d must divide N = %d"
                         % (n_samples, hop, N))
    return int(f.value), int(s.value)


def stream_state(B, N, hop, device):
    """A reset state buffer for B streams (uint8 on the device)."""
    nbytes = _capi.lib().drnmf_stream_state_bytes(int(B), int(N), int(hop))
    if nbytes == 0:
        raise ValueError("stream_state: B = %d must lie in [1, 65535], N = %d be a power of two in [64, 4096] and "
                         "hop = %d divide it" % (B, N, hop))
    state = torch.empty(nbytes, dtype=torch.uint8, device=device)
    stream_reset_enqueue(state, B, N, hop)
    return state


def stream_reset_enqueue(state, B, N, hop):
    _call("drnmf_stream_reset", _dev_index(state), int(B), int(N), int(hop), _capi.ptr(state), state.numel())


def stream_forward_enqueue(chunk, chunk_len_dev, final_dev, N, hop, mask_value, x, re, im, state):
    """drnmf_stream_forward on tensors the caller owns and has checked: enqueues, reads nothing back."""
    dev = _dev_index(chunk)
    B, stride = chunk.shape
    _call("drnmf_stream_forward", dev, B, stride, x.shape[1], int(N), int(hop), int(chunk.dtype == torch.int16),
          float(mask_value), _capi.ptr(chunk), _capi.ptr(chunk_len_dev), _capi.ptr(final_dev), _capi.ptr(x),
          _capi.ptr(re), _capi.ptr(im), _capi.ptr(state), state.numel())


def stream_inverse_enqueue(re, im, mask, N, hop, crop, y, state):
    """drnmf_stream_inverse on tensors the caller owns and has checked (y float32 or int16 [B, stride_y]):
    enqueues, reads nothing back."""
    dev = _dev_index(re)
    B, T, F = re.shape
    _call("drnmf_stream_inverse", dev, B, T, int(N), int(hop), _capi.ptr(re), _capi.ptr(im), _capi.ptr(mask),
          0 if mask is None else mask.stride(1), int(bool(crop)), int(y.dtype == torch.int16), _capi.ptr(y),
          y.shape[1], _capi.ptr(state), state.numel())


class WaveStream(object):
    """B independent streams through the streaming STFT / iSTFT: owns the state on the device and the host mirror
    of the counts.  A push is `analyse` (chunks -> the frames that have become complete), whatever turns their
    magnitude into a mask, then `synthesise` (-> the samples that have become final); every analyse that returns
    frames must be followed by one synthesise.  Frames and float32 samples are bitwise those of stft_ragged /
    istft_ragged on the whole signals, whatever the cuts."""

    def __init__(self, B, N, hop, mask_value=-1.0, device=None, crop=True):
        self.B, self.N, self.hop, self.crop = int(B), int(N), int(hop), bool(crop)
        self.mask_value = float(mask_value)
        dev = torch.device('cuda' if device is None else device)
        self.device = torch.device('cuda', _dev_of(dev))
        with torch.cuda.device(self.device):
            self.state = stream_state(self.B, self.N, self.hop, self.device)
        self._zero_counts()

    def _zero_counts(self):
        self.n_in = np.zeros(self.B, dtype=np.int64)          # samples pushed
        self.closed = np.zeros(self.B, dtype=bool)
        self.frames = np.zeros(self.B, dtype=np.int64)        # frames emitted
        self.samples = np.zeros(self.B, dtype=np.int64)       # samples emitted (or pending in _new_samples)
        self.dtype = None                                     # the chunks' type, fixed by the first push
        self._pending = None                                  # (T, new samples) between analyse and synthesise

    def reset(self):
        """Every stream fresh and open again."""
        with torch.cuda.device(self.device):
            stream_reset_enqueue(self.state, self.B, self.N, self.hop)
        self._zero_counts()

    def analyse(self, chunks, final=False):
        """chunks: B 1-D numpy arrays of one type (int16, scaled by 1/32768, or float32), any lengths, 0 included;
        final: a bool or B bools -- the stream ends with this chunk.  Returns (x, re, im, n_new): device tensors
        [B, T, N/2+1] with T = max(n_new), x holding mask_value behind a row's own n_new[b] frames, and the int64
        numpy counts.  The chunks, their lengths and the flags go up in one pinned copy."""
        B, N, hop = self.B, self.N, self.hop
        if self._pending is not None:
            raise ValueError("WaveStream.analyse: the previous push's frames have not been synthesised")
        rows = [np.asarray(c) for c in chunks]
        if len(rows) != B:
            raise ValueError("WaveStream.analyse: %d chunks for %d streams" % (len(rows), B))
        fin = np.broadcast_to(np.asarray(final, dtype=bool), (B,)) if np.ndim(final) == 0 else \
            np.asarray(list(final), dtype=bool)
        if fin.shape != (B,):
            raise ValueError("WaveStream.analyse: final must be a bool or %d bools" % B)
        dt = rows[0].dtype if self.dtype is None else self.dtype
        if dt not in (np.dtype('int16'), np.dtype('float32')):
            raise ValueError("WaveStream.analyse: chunks must be int16 or float32 (got %s)" % dt)
        for c in rows:
            if c.ndim != 1 or c.dtype != dt:
                raise ValueError("WaveStream.analyse: every chunk must be a 1-D %s array" % dt)
        lens = np.array([c.shape[0] for c in rows], dtype=np.int64)
        if np.any(self.closed & (lens > 0)):
            raise ValueError("WaveStream.analyse: stream %d is closed and takes only empty chunks until reset()"
                             % int(np.nonzero(self.closed & (lens > 0))[0][0]))
        n_in, closed = self.n_in + lens, self.closed | fin
        counts = [stream_counts(n_in[b], closed[b], N, hop, self.crop) for b in range(B)]
        frames = np.array([c[0] for c in counts], dtype=np.int64)
        samples = np.array([c[1] for c in counts], dtype=np.int64)
        n_new = frames - self.frames
        T = int(n_new.max())
        stride = max(1, int(lens.max()))
        # one pinned upload: lengths [B] int64 | flags [B] int32 | samples [B][stride]
        off = -(-(12 * B) // 16) * 16
        host = torch.empty(off + B * stride * dt.itemsize, dtype=torch.uint8, pin_memory=True)
        hn = host.numpy()
        hn[:8 * B].view(np.int64)[:] = lens
        hn[8 * B:12 * B].view(np.int32)[:] = fin
        pk = hn[off:].view(dt).reshape(B, stride)
        for b, c in enumerate(rows):
            pk[b, :c.shape[0]] = c
            pk[b, c.shape[0]:] = 0
        F = N // 2 + 1
        with torch.cuda.device(self.device):
            d = host.to(self.device, non_blocking=True)
            chunk = d[off:].view(torch.int16 if dt == np.dtype('int16') else torch.float32).view(B, stride)
            # (T = 0: the call still moves the carry on; its one row of frames is all padding)
            x = torch.empty((B, max(T, 1), F), dtype=torch.float32, device=self.device)
            re, im = torch.empty_like(x), torch.empty_like(x)
            stream_forward_enqueue(chunk, d[:8 * B].view(torch.int64), d[8 * B:12 * B].view(torch.int32), N, hop,
                                   self.mask_value, x, re, im, self.state)
        self.dtype = dt
        new_samples = samples - self.samples
        self.n_in, self.closed, self.frames, self.samples = n_in, closed, frames, samples
        if T == 0:
            return x[:, :0], re[:, :0], im[:, :0], n_new
        self._pending = (T, new_samples)
        return x, re, im, n_new

    def synthesise(self, re, im, mask, dtype='float32'):
        """The masked frames of the latest analyse back to samples: a list of B 1-D numpy arrays (float32, or
        int16 = truncation of 32767 * sample clamped to +-32767, WITHOUT util.wavwrite's peak normalisation),
        stream b's holding the samples that have become final.  mask [B, T, N/2+1] (the model's output, a padded
        row stride is taken in place) or None.  One copy down."""
        if dtype not in ('int16', 'float32'):
            raise ValueError("WaveStream.synthesise: dtype must be 'int16' or 'float32'")
        if self._pending is None:
            raise ValueError("WaveStream.synthesise: no analysed frames are pending")
        T, new_samples = self._pending
        B, F = self.B, self.N // 2 + 1
        if tuple(re.shape) != (B, T, F) or tuple(im.shape) != (B, T, F):
            raise ValueError("WaveStream.synthesise: re, im must be the [%d, %d, %d] tensors analyse returned"
                             % (B, T, F))
        re, im = _f32c(re, "re"), _f32c(im, "im")
        if mask is not None:
            if mask.dtype != torch.float32 or mask.device != re.device or tuple(mask.shape) != (B, T, F):
                raise ValueError("WaveStream.synthesise: mask must be float32 %s on %s" % ((B, T, F), re.device))
            if mask.stride(2) != 1 or mask.stride(1) < F or mask.stride(0) != T * mask.stride(1):
                mask = mask.contiguous()
        stride_y = max(1, int(new_samples.max()))
        tdt = torch.int16 if dtype == 'int16' else torch.float32
        with torch.cuda.device(self.device):
            y = torch.empty((B, stride_y), dtype=tdt, device=self.device)
            self._pending = None
            stream_inverse_enqueue(re, im, mask, self.N, self.hop, self.crop, y, self.state)
            back = torch.empty(y.shape, dtype=tdt, pin_memory=True)
            back.copy_(y, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        bn = back.numpy()
        return [bn[b, :int(new_samples[b])].copy() for b in range(B)]


# ---- STOI and the compute_scores row (score_audio.m:177-238; C ABI in include/drnmf_score.h) ---------------
STOI_BANDS = 15
SCORE_LABELS = ['SDR', 'SNR', 'SegSNR local', 'SegSNR global', 'PESQ', 'STOI']


def stoi_vad_frames(nsampl, fs):
    """Silence-detector frames of a signal of nsampl samples at fs (after resampling to 10 kHz)."""
    n = int(_capi.lib().drnmf_stoi_vad_frames(int(nsampl), int(fs)))
    if n < 0:
        raise ValueError("stoi: fs = %d is not supported (10000/fs reduced to p/q needs max(p, q) <= 160)" % fs)
    return n


def _host_lengths(lengths, n_sig, n):
    if lengths is None:
        return np.full(n_sig, n, dtype=np.int64)
    if isinstance(lengths, torch.Tensor):
        lengths = lengths.cpu().numpy()
    lh = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
    if lh.shape[0] != n_sig:
        raise ValueError("lengths has %d entries for %d signals" % (lh.shape[0], n_sig))
    return lh


def _stoi_pair_args(est, ref, lengths):
    est, ref = _f32c(est, "est"), _f32c(ref, "ref")
    if est.dim() == 1:
        est, ref = est[None], ref[None]
    if est.dim() != 2 or est.shape != ref.shape:
        raise ValueError("est and ref must have the same shape [n_sig, n] (got %s and %s)" %
                         (tuple(est.shape), tuple(ref.shape)))
    if ref.device != est.device:
        raise ValueError("est and ref must be on one device")
    return est, ref, _host_lengths(lengths, est.shape[0], est.shape[1])


def stoi(est, ref, fs=16000, lengths=None, return_parts=False, extended=False):
    """STOI per signal, as `stoi(xref, xest, fs)` of compute_scores (score_audio.m:231) [STOI-memory]:
    short-time objective intelligibility (Taal et al., 2011), restated in include/drnmf_score.h and
    tests/stoi_ref.py.  est, ref: device float32 [n_sig, n] (or 1-D); lengths: per-row valid samples (host
    ints or a tensor; default n).  Returns a float32 [n_sig] device tensor -- NaN for a row with fewer than 30
    band frames, as Matlab's mean of an empty set.  return_parts=True returns (stoi, parts), parts = dict(
    keep=[n_sig, V] bool silence decision on ref, env_ref / env_est=[n_sig, max(V-1, 1), 15] band envelopes
    (rows past a signal's own n_kept - 1 band frames are unspecified), n_kept=[n_sig] int64).
    extended=True is `estoi` with the same arguments: ESTOI, not STOI, comes back."""
    if extended:
        return estoi(est, ref, fs, lengths=lengths, return_parts=return_parts)
    di = _dev_index(est)
    est, ref, lh = _stoi_pair_args(est, ref, lengths)
    n_sig, n = est.shape
    max_len = int(lh.max()) if n_sig else 0
    V = stoi_vad_frames(max_len, fs)
    dev = est.device
    ws = _workspace(max(_capi.lib().drnmf_stoi_workspace_bytes(n_sig, max_len, int(fs)), 256), dev)
    out = torch.empty(n_sig, dtype=torch.float32, device=dev)
    keep = env_r = env_e = None
    if return_parts:
        keep = torch.zeros((n_sig, V), dtype=torch.uint8, device=dev)
        env_r = torch.zeros((n_sig, max(V - 1, 1), STOI_BANDS), dtype=torch.float32, device=dev)
        env_e = torch.zeros_like(env_r)
    _call("drnmf_stoi", di, n_sig, n, lh.ctypes.data_as(C.POINTER(C.c_int64)), int(fs), _capi.ptr(est),
          _capi.ptr(ref), _capi.ptr(out), _capi.ptr(keep if V > 0 else None), _capi.ptr(env_r), _capi.ptr(env_e),
          _capi.ptr(ws), ws.numel())
    if not return_parts:
        return out
    kb = keep.bool()
    return out, dict(keep=kb, env_ref=env_r, env_est=env_e, n_kept=kb.sum(dim=1))


def stoi_ext(est, ref, fs=16000, lengths=None, return_parts=False, want_stoi=True, want_estoi=True):
    """STOI and ESTOI of the same pairs from ONE drnmf_stoi_ext call (include/drnmf_estoi.h): resampling, the
    silence decision and the band envelopes run once, then each score's own last step.  Arguments as `stoi`.
    Returns (stoi, estoi), float32 [n_sig] device tensors, None for a score not wanted; stoi has the bits `stoi`
    returns.  return_parts=True appends `stoi`'s parts plus d_ext=[n_sig, max(V - 30, 1)] float64, the ESTOI of
    each 30-frame segment (entries past a signal's own n_kept - 30 segments are unspecified)."""
    if not (want_stoi or want_estoi):
        raise ValueError("stoi_ext: nothing to compute (want_stoi and want_estoi are both False)")
    di = _dev_index(est)
    est, ref, lh = _stoi_pair_args(est, ref, lengths)
    n_sig, n = est.shape
    max_len = int(lh.max()) if n_sig else 0
    V = stoi_vad_frames(max_len, fs)
    dev = est.device
    ws = _workspace(max(_capi.lib().drnmf_stoi_ext_workspace_bytes(n_sig, max_len, int(fs)), 256), dev)
    out_s = torch.empty(n_sig, dtype=torch.float32, device=dev) if want_stoi else None
    out_e = torch.empty(n_sig, dtype=torch.float32, device=dev) if want_estoi else None
    keep = env_r = env_e = d_ext = None
    if return_parts:
        keep = torch.zeros((n_sig, V), dtype=torch.uint8, device=dev)
        env_r = torch.zeros((n_sig, max(V - 1, 1), STOI_BANDS), dtype=torch.float32, device=dev)
        env_e = torch.zeros_like(env_r)
        d_ext = torch.zeros((n_sig, max(V - 30, 1)), dtype=torch.float64, device=dev)
    _call("drnmf_stoi_ext", di, n_sig, n, lh.ctypes.data_as(C.POINTER(C.c_int64)), int(fs), _capi.ptr(est),
          _capi.ptr(ref), _capi.ptr(out_s), _capi.ptr(out_e), _capi.ptr(keep if V > 0 else None), _capi.ptr(env_r),
          _capi.ptr(env_e), _capi.ptr(d_ext), _capi.ptr(ws), ws.numel())
    if not return_parts:
        return out_s, out_e
    kb = keep.bool()
    return out_s, out_e, dict(keep=kb, env_ref=env_r, env_est=env_e, n_kept=kb.sum(dim=1), d_ext=d_ext)


def estoi(est, ref, fs=16000, lengths=None, return_parts=False):
    """ESTOI per signal [ESTOI-memory]: the extended STOI of Jensen & Taal (IEEE/ACM TASLP 24(11), 2016), which
    unlike STOI sees temporally modulated maskers; restated in include/drnmf_estoi.h and tests/estoi_ref.py.  STOI's
    band envelopes, then every 15 x 30 segment of each is normalised (mean and norm) along time, then along the
    bands; a segment scores the sum of the products / 30, a signal the mean over its segments.  Arguments and
    return as `stoi`: float32 [n_sig] on the device, NaN below 30 band frames; the parts are `stoi`'s plus
    d_ext=[n_sig, max(V - 30, 1)] float64 (see `stoi_ext`).  Plain arithmetic, no epsilon: a zero norm is
    0 / 0, so a band constant over 30 frames or a digitally silent stretch of the estimate gives NaN for the
    signal (an all-zero estimate: STOI 1, ESTOI NaN); a signal against itself gives 1."""
    res = stoi_ext(est, ref, fs, lengths=lengths, return_parts=return_parts, want_stoi=False)
    return (res[1], res[2]) if return_parts else res[1]


def compute_scores(est, ref, fs, lengths_est=None, lengths_ref=None, flen=512, sdr_solver="host", extended=False):
    """One row per file as compute_scores (score_audio.m:177-238) returns it:
        S = [SDR, SNR, SegSNR local, SegSNR global, PESQ, STOI]        (score_audio.m:233-236)
    est [n_sig, n_est], ref [n_sig, n_ref]: device float32 (or 1-D), each row valid up to its length
    (default: the row width).  Each pair is truncated to min(len_est, len_ref); SDR (`sdr_db`, 512-tap BSS Eval)
    and SNR (`snr_db`) see the pairs zero-padded to a common width, to which both are neutral; STOI (`stoi`) runs
    at fs on the truncated pairs.  Returns (S, labels): S float64 numpy [n_sig, 6], labels SCORE_LABELS.
    sdr_solver="device": SDR runs over each pair's own length with the normal equations solved on the device
    (`sdr_db(..., lengths=, solver="device")`), nothing waits for the host between the three scores, and all
    columns come down in one copy.
    extended=True appends a seventh column, ESTOI (`estoi`; not a column of the reference's row): S is
    [n_sig, 7], labels SCORE_LABELS + ['ESTOI'], and STOI and ESTOI come from one `stoi_ext` call on the truncated
    pairs.  The first six columns are those of extended=False.

    SegSNR and PESQ are NaN.  SegSNR is voicebox `snrseg` (score_audio.m:212), whose default mode runs a P.56
    speech-activity detector and a sub-sample delay search whose exact definitions are not available to this
    project; PESQ is ITU-T P.862, large, table-driven and licensed.  A restatement from memory would be a number
    labelled as the reference's that is probably not the reference's, so neither column is computed."""
    if sdr_solver not in SDR_SOLVERS:
        raise ValueError("compute_scores: sdr_solver must be one of %s (got %r)" % (SDR_SOLVERS, sdr_solver))
    if est.dim() == 1:
        est, ref = est[None], ref[None]
    if est.dim() != 2 or ref.dim() != 2 or est.shape[0] != ref.shape[0]:
        raise ValueError("est and ref must be [n_sig, n] with the same n_sig (got %s and %s)" %
                         (tuple(est.shape), tuple(ref.shape)))
    n_sig = est.shape[0]
    le = _host_lengths(lengths_est, n_sig, est.shape[1])
    lr = _host_lengths(lengths_ref, n_sig, ref.shape[1])
    if np.any(le > est.shape[1]) or np.any(lr > ref.shape[1]) or np.any(le < 0) or np.any(lr < 0):
        raise ValueError("lengths outside [0, row width]")
    ln = np.minimum(le, lr)
    width = max(int(ln.max()) if n_sig else 0, 1)
    col = torch.arange(width, device=est.device)[None, :]
    valid = col < torch.from_numpy(ln).to(est.device)[:, None]
    e = torch.zeros((n_sig, width), dtype=torch.float32, device=est.device)
    r = torch.zeros_like(e)
    we, wr = min(width, est.shape[1]), min(width, ref.shape[1])
    e[:, :we] = _f32c(est, "est")[:, :we]
    r[:, :wr] = _f32c(ref, "ref")[:, :wr]
    e = torch.where(valid, e, torch.zeros_like(e))
    r = torch.where(valid, r, torch.zeros_like(r))
    labels = list(SCORE_LABELS) + (['ESTOI'] if extended else [])
    S = np.full((n_sig, len(labels)), np.nan, dtype=np.float64)

    def intelligibility():          # [STOI] or [STOI, ESTOI], device tensors
        return list(stoi_ext(e, r, fs=fs, lengths=ln)) if extended else [stoi(e, r, fs=fs, lengths=ln)]

    if sdr_solver == "device":
        cols = torch.stack([sdr_db(e, r, flen=flen, lengths=ln, solver="device"), snr_db(e, r)] +
                           intelligibility()).cpu().numpy()
        S[:, 0], S[:, 1], S[:, 5:] = cols[0], cols[1], cols[2:].T
        return S, labels
    S[:, 0] = sdr_db(e, r, flen=flen).cpu().numpy()
    S[:, 1] = snr_db(e, r).cpu().numpy()
    S[:, 5:] = torch.stack(intelligibility()).cpu().numpy().T
    return S, labels


# ---- LSTM baseline (build_lstm, enhance.py:321-345; C ABI in include/drnmf_lstm.h) -----------------------
LSTM_ACTIVATIONS = {"hard_sigmoid": _capi.ACTIVATIONS["hard_sigmoid"], "sigmoid": _capi.ACTIVATIONS["sigmoid"]}


def make_lstm_desc(B, T, F, H, K, recurrent_activation="hard_sigmoid", *, operand_f16=False):
    """operand_f16: fp16 operands in the recurrent products (inference only; drnmf_lstm_desc_t.operand_f16).  The
    prepared block and the workspace depend on it: prepare, forward and head take descriptors that agree."""
    if recurrent_activation not in LSTM_ACTIVATIONS:
        raise ValueError("recurrent_activation must be one of %s" % sorted(LSTM_ACTIVATIONS))
    return _capi.LstmDesc(int(B), int(T), int(F), int(H), int(K), LSTM_ACTIVATIONS[recurrent_activation],
                          1 if operand_f16 else 0)


def lstm_prepare_params(desc, kernels, recurrents, biases, w_out, b_out, out=None):
    """Keras layouts: kernels = [kernel_0 [F,4H], kernel_1..K-1 [H,4H]], recurrents [K] x [H,4H], biases [K] x [4H],
    w_out [H,F], b_out [F] (device tensors) -> prepared block (uint8)."""
    K, H, F = desc.K, desc.H, desc.F
    if len(kernels) != K or len(recurrents) != K or len(biases) != K:
        raise ValueError("lstm_prepare_params: K = %d kernels / recurrent kernels / biases expected" % K)
    k0 = _f32c(kernels[0], "kernel_0")
    dev = _dev_index(k0)
    if tuple(k0.shape) != (F, 4 * H):
        raise ValueError("kernel_0 must have shape (F,4H) = (%d,%d)" % (F, 4 * H))
    for k in range(1, K):
        if tuple(kernels[k].shape) != (H, 4 * H):
            raise ValueError("kernel_%d must have shape (H,4H) = (%d,%d)" % (k, H, 4 * H))
    for k in range(K):
        if tuple(recurrents[k].shape) != (H, 4 * H) or tuple(biases[k].shape) != (4 * H,):
            raise ValueError("recurrent_kernel / bias of layer %d must have shapes (H,4H) / (4H,)" % k)
    rest = _f32c(torch.stack([t.float() for t in kernels[1:]]), "kernel_rest") if K > 1 else None
    rec = _f32c(torch.stack([t.float() for t in recurrents]), "recurrent_kernel")
    bias = _f32c(torch.stack([t.float() for t in biases]), "bias")
    w_out, b_out = _f32c(w_out, "w_out"), _f32c(b_out, "b_out")
    if tuple(w_out.shape) != (H, F) or tuple(b_out.shape) != (F,):
        raise ValueError("w_out / b_out must have shapes (H,F) / (F,) = (%d,%d) / (%d,)" % (H, F, F))
    out = _workspace(_capi.lib().drnmf_lstm_params_bytes(C.byref(desc)), k0.device, out)
    _call("drnmf_lstm_prepare_params", dev, C.byref(desc), _capi.ptr(k0), _capi.ptr(rest), _capi.ptr(rec),
          _capi.ptr(bias), _capi.ptr(w_out), _capi.ptr(b_out), _capi.ptr(out), out.numel())
    return out


def lstm_workspace(desc, device):
    nbytes = _capi.lib().drnmf_lstm_workspace_bytes(C.byref(desc))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def lstm_hidden_ld(H):
    """Row stride of the hidden buffers lstm_forward allocates: round_up(H, 4) (the head's vectorised path)."""
    return (int(H) + 3) // 4 * 4


def _hidden_ld(t, desc, what):
    """Row stride of a (B,T,H) float32 tensor whose rows may be padded: t.stride() == (T*ld, ld, 1), ld >= H."""
    if t.dtype != torch.float32 or tuple(t.shape) != (desc.B, desc.T, desc.H):
        raise ValueError("%s must be a (B,T,H) = (%d,%d,%d) float32 tensor" % (what, desc.B, desc.T, desc.H))
    ld = t.stride(1)
    if t.stride(2) != 1 or ld < desc.H or (desc.B > 1 and t.stride(0) != desc.T * ld):
        raise ValueError("%s must have strides (T*ld, ld, 1) with ld >= H" % what)
    return int(ld)


def _lstm_state_pair(state, desc, what, device):
    """`state`: None, or (h, c) of contiguous float32 [K,B,H] device tensors, either of which may be None (the C
    ABI's NULL: zeros on the way in, not wanted on the way out)."""
    if state is None:
        return None, None
    if not isinstance(state, (tuple, list)) or len(state) != 2:
        raise ValueError("%s must be a pair (h, c)" % what)
    # (h and c go by the pair's name: no string is built per call on the streaming path)
    _check_state(state[0], (desc.K, desc.B, desc.H), device, what)
    _check_state(state[1], (desc.K, desc.B, desc.H), device, what)
    return state[0], state[1]


def _lstm_forward_call(entry, x, mask_value, params, desc, out, workspace, initial_state, final_state):
    """lstm_forward and lstm_train_forward: the C entry `entry`, or `entry`_stateful when a state is given."""
    dev = _dev_index(x)
    x = _f32c(x, "x")
    if tuple(x.shape) != (desc.B, desc.T, desc.F):
        raise ValueError("x has shape %s, descriptor says (%d,%d,%d)" % (tuple(x.shape), desc.B, desc.T, desc.F))
    if out is None:
        ld = lstm_hidden_ld(desc.H)
        out = torch.empty((desc.B, desc.T, ld), dtype=torch.float32, device=x.device)[..., :desc.H]
    else:
        ld = _hidden_ld(out, desc, "out")       # (rows may be padded: not `_out`'s contiguous test)
    mv = _mask_nan(mask_value)
    tail = (_capi.ptr(out), ld, _capi.ptr(workspace), workspace.numel())
    if initial_state is not None or final_state is not None:
        ih, ic = _lstm_state_pair(initial_state, desc, "initial_state", x.device)
        fh, fc = _lstm_state_pair(final_state, desc, "final_state", x.device)
        _call(entry + "_stateful", dev, C.byref(desc), _capi.ptr(x), mv, _capi.ptr(params), _capi.ptr(ih),
              _capi.ptr(ic), _capi.ptr(fh), _capi.ptr(fc), *tail)
    else:
        _call(entry, dev, C.byref(desc), _capi.ptr(x), mv, _capi.ptr(params), *tail)
    return out


def lstm_forward(x, mask_value, params, desc, out=None, workspace=None, *, initial_state=None, final_state=None):
    """K stacked Keras LSTM layers (return_sequences=True) behind Masking(mask_value): x [B,T,F] -> the last
    layer's outputs [B,T,H], by default a view of a [B,T,lstm_hidden_ld(H)] buffer whose padding columns the
    kernel zeroes (`out`: any (B,T,H) tensor with strides (T*ld, ld, 1)).  mask_value None: no frame is masked.
    initial_state / final_state: (h, c) pairs of [K,B,H] tensors, the state entering frame 0 (None: zeros) and the
    one leaving frame T-1, written in place (None: not wanted); the same pair may be passed as both
    (drnmf_lstm_forward_stateful).  Both None: drnmf_lstm_forward."""
    if workspace is None:
        workspace = lstm_workspace(desc, x.device)
    return _lstm_forward_call("drnmf_lstm_forward", x, mask_value, params, desc, out, workspace, initial_state,
                              final_state)


def lstm_head_forward(hidden, params, desc, out=None):
    """TimeDistributed(Dense(F)) + sigmoid on every frame: hidden [B,T,H] -> [B,T,F].  hidden: contiguous, or
    rows padded to a stride ld as lstm_forward returns them (padding columns finite)."""
    dev = _dev_index(hidden)
    ld = _hidden_ld(hidden, desc, "hidden")
    out = _out(out, (desc.B, desc.T, desc.F), torch.float32, hidden.device)
    _call("drnmf_lstm_head_forward", dev, C.byref(desc), _capi.ptr(hidden), ld, _capi.ptr(params), _capi.ptr(out))
    return out


# ---- LSTM training (include/drnmf_lstm.h: drnmf_lstm_train_* / loss_head_backward / backward) ------------------
def lstm_train_workspace(desc, device):
    """The workspace the three training calls share (its size grows with B and T)."""
    nbytes = _capi.lib().drnmf_lstm_train_workspace_bytes(C.byref(desc))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def lstm_train_forward(x, mask_value, params, desc, workspace, out=None, *, initial_state=None, final_state=None):
    """lstm_forward (the same hidden states, bit for bit) that also keeps in `workspace` what
    lstm_loss_head_backward and lstm_backward need.  initial_state / final_state as in lstm_forward
    (drnmf_lstm_train_forward_stateful): the entering state is kept in the workspace as a constant of the gradient,
    which lstm_backward then reads there."""
    return _lstm_forward_call("drnmf_lstm_train_forward", x, mask_value, params, desc, out, workspace, initial_state,
                              final_state)


def lstm_loss_head_backward(y, w, hidden, params, w_out, desc, workspace, sums, d_hidden, d_w_out, d_b_out):
    """Loss 'mse_of_masked' and the head's backward after lstm_train_forward on the same workspace: writes
    sums [2] = {sum w * mean_F (xm*s - y)^2, #frames with w != 0} (unnormalised), d_hidden [B,T,H], d_w_out [H,F],
    d_b_out [F] (device tensors, overwritten)."""
    dev = _dev_index(hidden)
    y, w, w_out = _f32c(y, "y"), _f32c(w, "sample_weight"), _f32c(w_out, "w_out")
    if tuple(y.shape) != (desc.B, desc.T, desc.F) or tuple(w.shape) != (desc.B, desc.T):
        raise ValueError("y / sample_weight must have shapes (B,T,F) / (B,T)")
    ld = _hidden_ld(hidden, desc, "hidden")
    for t, shp, what in ((sums, (2,), "sums"), (d_hidden, (desc.B, desc.T, desc.H), "d_hidden"),
                         (d_w_out, (desc.H, desc.F), "d_w_out"), (d_b_out, (desc.F,), "d_b_out")):
        _given(t, shp, torch.float32, hidden.device, what)
    _call("drnmf_lstm_loss_head_backward", dev, C.byref(desc), _capi.ptr(y), _capi.ptr(w), _capi.ptr(hidden), ld,
          _capi.ptr(params), _capi.ptr(w_out), _capi.ptr(sums), _capi.ptr(d_hidden), _capi.ptr(d_w_out),
          _capi.ptr(d_b_out), _capi.ptr(workspace), workspace.numel())


def _ptr_array(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])


def lstm_backward(kernels, recurrents, d_hidden, d_kernels, d_recurrents, d_biases, desc, workspace):
    """BPTT after lstm_loss_head_backward on the same workspace: the unnormalised gradients of every layer's
    kernel, recurrent_kernel and bias, written in Keras layout into the given (contiguous float32) tensors."""
    dev = _dev_index(d_hidden)
    K, H, F = desc.K, desc.H, desc.F
    if not (len(kernels) == len(recurrents) == len(d_kernels) == len(d_recurrents) == len(d_biases) == K):
        raise ValueError("lstm_backward: K = %d tensors per list expected" % K)
    for k in range(K):
        fin = F if k == 0 else H
        for t, shp, what in ((kernels[k], (fin, 4 * H), "lstm_backward: kernels[k]"),
                             (recurrents[k], (H, 4 * H), "lstm_backward: recurrents[k]"),
                             (d_kernels[k], (fin, 4 * H), "lstm_backward: d_kernels[k]"),
                             (d_recurrents[k], (H, 4 * H), "lstm_backward: d_recurrents[k]"),
                             (d_biases[k], (4 * H,), "lstm_backward: d_biases[k]")):
            _given(t, shp, torch.float32, d_hidden.device, what)
    _given(d_hidden, (desc.B, desc.T, H), torch.float32, d_hidden.device, "d_hidden")
    _call("drnmf_lstm_backward", dev, C.byref(desc), _ptr_array(kernels), _ptr_array(recurrents),
          _capi.ptr(d_hidden), _ptr_array(d_kernels), _ptr_array(d_recurrents), _ptr_array(d_biases),
          _capi.ptr(workspace), workspace.numel())


# ---- waveform losses (include/drnmf_waveloss.h) ----------------------------------------------------------------
WAVE_LOSSES = _capi.WAVE_LOSSES


def _wave_kind(loss, what):
    if loss not in WAVE_LOSSES:
        raise ValueError("%s: loss must be one of %s (got %r)" % (what, sorted(WAVE_LOSSES), loss))
    return WAVE_LOSSES[loss]


def istft_ragged_vjp_enqueue(g, re, im, lengths_dev, sig_index_dev, N, hop, crop, d_mask):
    """drnmf_istft_ragged_vjp on tensors the caller owns and has checked: enqueues, reads nothing back."""
    dev = _dev_index(re)
    b, T, F = re.shape
    _call("drnmf_istft_ragged_vjp", dev, g.shape[0], b, T, int(N), int(hop), _capi.ptr(lengths_dev),
          _capi.ptr(sig_index_dev), _capi.ptr(re), _capi.ptr(im), _capi.ptr(g), g.shape[1], int(bool(crop)),
          _capi.ptr(d_mask), d_mask.stride(1))


def istft_ragged_vjp(g, re, im, lengths, N, hop, sig_index=None, crop=False, out=None):
    """Transpose of `istft_ragged` with respect to its mask: g [n_sig, width] float32, row sig_index[k] the cotangent
    of slab row k's reconstruction (samples at or behind ragged_out_lengths(lengths, N, hop, crop) count as 0 and
    are not read); re, im [b, T, N/2+1] as `stft_ragged` returned them.  Returns d_mask [b, T, N/2+1] (`out`: a
    contiguous tensor of that shape): zeros in the frames behind a row's own.  A row's result is bitwise the same
    in any batch."""
    F = N // 2 + 1
    if re.dim() != 3 or re.shape != im.shape or re.shape[2] != F:
        raise ValueError("istft_ragged_vjp: re, im must be [b, T, %d] (got %s, %s)" % (F, tuple(re.shape),
                                                                                      tuple(im.shape)))
    dev = re.device
    _dev_index(re)
    re, im = _f32c(re, "re"), _f32c(im, "im")
    if g.dim() != 2 or g.dtype != torch.float32 or g.device != dev or im.device != dev:
        raise ValueError("istft_ragged_vjp: g must be [n_sig, width] float32 on %s" % (dev,))
    if int(hop) < 1:
        raise ValueError("istft_ragged_vjp: hop < 1")
    g = g.contiguous()
    n_sig = g.shape[0]
    b, T, _ = re.shape
    _, ld = _ragged_lengths(lengths, n_sig, 1 << 40, dev, "istft_ragged_vjp")
    idx = _ragged_index(sig_index, n_sig, dev, "istft_ragged_vjp")
    if idx.numel() != b:
        raise ValueError("istft_ragged_vjp: %d slab rows but sig_index names %d" % (b, idx.numel()))
    out = _out(out, (b, T, F), torch.float32, dev, "istft_ragged_vjp: out")
    istft_ragged_vjp_enqueue(g, re, im, ld, idx, N, hop, crop, out)
    return out


def wave_loss_workspace(n_sig, width, device, have=None):
    return _workspace(_capi.lib().drnmf_wave_loss_workspace_bytes(int(n_sig), int(width)), device, have)


def wave_loss_enqueue(est, ref, lengths_dev, kind, loss, counted, g, sums, workspace):
    """drnmf_wave_loss on tensors the caller owns and has checked: enqueues, reads nothing back."""
    n_sig, width = est.shape
    _call("drnmf_wave_loss", _dev_index(est), n_sig, width, _capi.ptr(lengths_dev), _capi.ptr(est), _capi.ptr(ref),
          int(kind), _capi.ptr(loss), _capi.ptr(counted), _capi.ptr(g), _capi.ptr(sums), _capi.ptr(workspace),
          workspace.numel())


def wave_loss(est, ref, lengths, loss='si_sdr', out=None, workspace=None):
    """Per-row waveform loss between est and ref [n_sig, width] float32, row i valid up to lengths[i] (host ints
    or a tensor, each in [1, width]).  loss 'wave_mse': mean (est - ref)^2 over the row; 'si_sdr': minus the
    scale-invariant SDR in dB, -10 log10((p^2/q + eps) / (e - p^2/q + eps)), a row whose reference is digitally
    silent not counted (loss 0, gradient 0).  Returns (loss [n_sig], counted [n_sig] (1 / 0), g [n_sig, width],
    sums [2] = {sum of counted losses, their number}) on the device; g is the gradient of that SUM with respect
    to est, zeros behind a row's length.  `out`: that 4-tuple to write into."""
    kind = _wave_kind(loss, "wave_loss")
    if est.dim() != 2 or est.shape != ref.shape or est.dtype != torch.float32 or ref.dtype != torch.float32 or \
            est.device != ref.device:
        raise ValueError("wave_loss: est, ref must be float32 [n_sig, width] on one device (got %s %s, %s %s)" %
                         (est.dtype, tuple(est.shape), ref.dtype, tuple(ref.shape)))
    dev = est.device
    _dev_index(est)
    est, ref = est.contiguous(), ref.contiguous()
    n_sig, width = est.shape
    if n_sig < 1 or width < 1:
        raise ValueError("wave_loss: empty batch")
    _, ld = _ragged_lengths(lengths, n_sig, width, dev, "wave_loss")
    lo, co, g, sums = (None, None, None, None) if out is None else out
    lo = _out(lo, (n_sig,), torch.float32, dev, "wave_loss: loss")
    co = _out(co, (n_sig,), torch.float32, dev, "wave_loss: counted")
    g = _out(g, (n_sig, width), torch.float32, dev, "wave_loss: g")
    sums = _out(sums, (2,), torch.float32, dev, "wave_loss: sums")
    wave_loss_enqueue(est, ref, ld, kind, lo, co, g, sums, wave_loss_workspace(n_sig, width, dev, workspace))
    return lo, co, g, sums


# ---- the STOI criterion (include/drnmf_stoi_loss.h) -----------------------------------------------------------------
WAVE_CRITERIA = tuple(sorted(WAVE_LOSSES)) + ('stoi',)     # what train_on_wavs / test_on_wavs / fit_waveform take


def _wave_criterion(loss, what):
    if loss not in WAVE_CRITERIA:
        raise ValueError("%s: loss must be one of %s (got %r)" % (what, list(WAVE_CRITERIA), loss))
    return loss


def stoi_loss_workspace(n_sig, max_len, fs, device, have=None):
    return _workspace(max(_capi.lib().drnmf_stoi_loss_workspace_bytes(int(n_sig), int(max_len), int(fs)), 256),
                      device, have)


def stoi_loss_enqueue(est, ref, lengths_host, fs, loss, counted, g, sums, workspace):
    """drnmf_stoi_loss on tensors the caller owns and has checked (lengths_host: a contiguous int64 numpy array):
    enqueues, reads nothing back."""
    n_sig, width = est.shape
    _call("drnmf_stoi_loss", _dev_index(est), n_sig, width, lengths_host.ctypes.data_as(C.POINTER(C.c_int64)), int(fs),
          _capi.ptr(est), _capi.ptr(ref), _capi.STOI_LOSS_STOI, _capi.ptr(loss), _capi.ptr(counted), _capi.ptr(g),
          _capi.ptr(sums), _capi.ptr(workspace), workspace.numel())


def stoi_loss(est, ref, lengths, fs=16000, out=None, workspace=None):
    """Minus STOI per row and its exact gradient (include/drnmf_stoi_loss.h, tests/stoi_loss_ref.py): est, ref
    [n_sig, width] float32 on one device, row i valid up to lengths[i] (host ints or a tensor; None: width).  Returns
    (loss [n_sig], counted [n_sig] (1 / 0), g [n_sig, width], sums [2] = {sum of counted losses, their number}) on
    the device, shaped and typed as `wave_loss` returns them; loss has the bits of -`stoi`; g is the gradient of
    that SUM with respect to est, zeros behind a row's length.  A row whose STOI is not finite (fewer than 30 band
    frames -- about 0.41 s at 16 kHz -- or a zero-variance band) is not counted: loss 0, gradient 0.  A segment-band
    whose estimate is digitally silent scores 1 and gives no gradient; a zero band envelope passes none on.  The
    silence decision comes from ref alone, so nothing flows through it.  A row's results are bitwise the same in any
    batch.  `out`: that 4-tuple to write into."""
    if est.dim() != 2 or est.shape != ref.shape or est.dtype != torch.float32 or ref.dtype != torch.float32 or \
            est.device != ref.device:
        raise ValueError("stoi_loss: est, ref must be float32 [n_sig, width] on one device (got %s %s, %s %s)" %
                         (est.dtype, tuple(est.shape), ref.dtype, tuple(ref.shape)))
    dev = est.device
    _dev_index(est)
    est, ref = est.contiguous(), ref.contiguous()
    n_sig, width = est.shape
    if n_sig < 1 or width < 1:
        raise ValueError("stoi_loss: empty batch")
    lh = _host_lengths(lengths, n_sig, width)
    if lh.min() < 0 or lh.max() > width:
        raise ValueError("stoi_loss: lengths must lie in [0, %d]" % width)
    max_len = int(lh.max())
    stoi_vad_frames(max_len, fs)                               # (raises for an unsupported fs)
    lo, co, g, sums = (None, None, None, None) if out is None else out
    lo = _out(lo, (n_sig,), torch.float32, dev, "stoi_loss: loss")
    co = _out(co, (n_sig,), torch.float32, dev, "stoi_loss: counted")
    g = _out(g, (n_sig, width), torch.float32, dev, "stoi_loss: g")
    sums = _out(sums, (2,), torch.float32, dev, "stoi_loss: sums")
    stoi_loss_enqueue(est, ref, lh, fs, lo, co, g, sums, stoi_loss_workspace(n_sig, max_len, fs, dev, workspace))
    return lo, co, g, sums


def _cot_ld(d_mask, shape, dev, what):
    """Row stride of a mask cotangent [..., F] whose rows may be padded (strides (.., ld, 1), ld >= F)."""
    if d_mask.dtype != torch.float32 or tuple(d_mask.shape) != shape or d_mask.device != dev:
        raise ValueError("%s: d_mask must be a float32 tensor of shape %s on %s (got %s %s on %s)" %
                         (what, shape, dev, d_mask.dtype, tuple(d_mask.shape), d_mask.device))
    ld = d_mask.stride(-2) if d_mask.dim() >= 2 else shape[-1]
    ok = d_mask.stride(-1) == 1 and ld >= shape[-1]
    for i in range(d_mask.dim() - 3, -1, -1):
        ok = ok and (d_mask.shape[i] == 1 or d_mask.stride(i) == d_mask.stride(i + 1) * d_mask.shape[i + 1])
    return (d_mask, int(ld)) if ok else (d_mask.contiguous(), shape[-1])


def head_backward_cot(d_mask, hidden, kernel_clean, kernel_noise, A, Bn, square=False, h_off=0, out=None,
                      workspace=None):
    """The mask head's backward for a given cotangent of the mask (drnmf_head_backward_cot): d_mask [..., F]
    (rows may be padded), hidden [..., ld], A, Bn [..., F] as head_forward(want_ab=True) returned them.  Returns
    (d_hidden [..., 2r], d_kernel_clean, d_kernel_noise); `out` = (d_kernel_clean, d_kernel_noise) to write
    into."""
    di = _dev_index(hidden)
    hidden, A, Bn = (_f32c(t, n) for t, n in ((hidden, "hidden"), (A, "A"), (Bn, "Bn")))
    kc, kn = _f32c(kernel_clean, "kernel_clean"), _f32c(kernel_noise, "kernel_noise")
    r, F = kc.shape
    if tuple(kn.shape) != (r, F):
        raise ValueError("kernel_noise shape %s != kernel_clean shape %s" % (tuple(kn.shape), (r, F)))
    ld = hidden.shape[-1]
    rows = hidden.numel() // ld
    dev = hidden.device
    if h_off < 0 or ld < h_off + 2 * r or A.numel() != rows * F or Bn.numel() != rows * F:
        raise ValueError("head_backward_cot: shape mismatch")
    d_mask, ld_dm = _cot_ld(d_mask, tuple(hidden.shape[:-1]) + (F,), dev, "head_backward_cot")
    dkc, dkn = (None, None) if out is None else out
    dkc = _out(dkc, (r, F), torch.float32, dev, "d_kernel_clean")
    dkn = _out(dkn, (r, F), torch.float32, dev, "d_kernel_noise")
    d_hidden = torch.empty(tuple(hidden.shape[:-1]) + (2 * r,), dtype=torch.float32, device=dev)
    ws = _workspace(_capi.lib().drnmf_loss_head_workspace_bytes(rows, F, r), dev, workspace)
    _call("drnmf_head_backward_cot", di, rows, F, r, _capi.ptr(hidden), ld, int(h_off), _capi.ptr(kc), _capi.ptr(kn),
          int(bool(square)), _capi.ptr(A), _capi.ptr(Bn), _capi.ptr(d_mask), ld_dm, _capi.ptr(d_hidden),
          _capi.ptr(dkc), _capi.ptr(dkn), _capi.ptr(ws), ws.numel())
    return d_hidden, dkc, dkn


def lstm_head_backward_cot(d_mask, hidden, params, w_out, desc, workspace, d_hidden, d_w_out, d_b_out):
    """The sigmoid head's backward for a given cotangent d_mask [B,T,F] of its output, after lstm_train_forward on
    the same workspace: writes d_hidden [B,T,H], d_w_out [H,F], d_b_out [F] (device tensors, overwritten)."""
    dev = _dev_index(hidden)
    if desc.operand_f16:
        raise ValueError("lstm_head_backward_cot: operand_f16 descriptors are inference only")
    w_out = _f32c(w_out, "w_out")
    ld = _hidden_ld(hidden, desc, "hidden")
    d_mask, ld_dm = _cot_ld(d_mask, (desc.B, desc.T, desc.F), hidden.device, "lstm_head_backward_cot")
    for t, shp, what in ((d_hidden, (desc.B, desc.T, desc.H), "d_hidden"), (d_w_out, (desc.H, desc.F), "d_w_out"),
                         (d_b_out, (desc.F,), "d_b_out")):
        _given(t, shp, torch.float32, hidden.device, what)
    _call("drnmf_lstm_head_backward_cot", dev, C.byref(desc), _capi.ptr(d_mask), ld_dm, _capi.ptr(hidden), ld,
          _capi.ptr(params), _capi.ptr(w_out), _capi.ptr(d_hidden), _capi.ptr(d_w_out), _capi.ptr(d_b_out),
          _capi.ptr(workspace), workspace.numel())
