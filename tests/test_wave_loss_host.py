"""CPU-side tests of the waveform criteria: the fp64 reference of tests/wave_loss_ref.py against the oracle's
reconstruction (the dot-product identity of the transposed inverse) and against autograd of the loss definitions,
the C ABI of include/drnmf_waveloss.h and its argument validation on a handle bound to no device, and the checks
the Python layers make before they touch a device (no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import wave_loss_ref as R
from oracle import drnmf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_waveloss.h")
NAMES = {"drnmf_istft_ragged_vjp", "drnmf_wave_loss_workspace_bytes", "drnmf_wave_loss", "drnmf_head_backward_cot",
         "drnmf_lstm_head_backward_cot"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


# ---- the reference against the oracle and against autograd ------------------------------------------------------
@pytest.mark.parametrize("crop", [False, True], ids=["full", "crop"])
@pytest.mark.parametrize("N,hop", R.VJP_SIZES, ids=["%dx%d" % s for s in R.VJP_SIZES])
def test_dot_product_identity_of_the_transposed_inverse(N, hop, crop):
    """<g, reconstruct(m)> = <vjp(g), m> for random g and m: the inverse is linear in the mask, so the identity at
    random vectors pins the transpose.  1e-12 relative to the sum of the absolute terms' larger side."""
    rng = np.random.default_rng(N + hop + int(crop))
    w = O.sqrt_hann(N)
    for n in R.vjp_lengths(N, hop):
        x = rng.standard_normal(n)
        S = O.stft_mc(x, N, hop, w)
        nf = S.shape[1]
        assert nf == R.frames(n, N, hop)
        m = rng.random((nf, N // 2 + 1))
        n_out = R.out_length(n, N, hop, crop)
        y = O.reconstruct(S.real, S.imag, m.T, hop, w, n if crop else None)
        assert y.shape[0] == n_out
        g = rng.standard_normal(n_out + 3)                         # (the samples behind n_out do not count)
        d = R.vjp(S.real.T, S.imag.T, g, N, hop, n_out)
        lhs, rhs = float(g[:n_out] @ y), float(np.sum(d * m))
        scale = max(float(np.abs(g[:n_out]) @ np.abs(y)), 1e-300)
        assert abs(lhs - rhs) <= 1e-12 * scale, (n, lhs, rhs)
        # the differentiable restatement the end-to-end references use is the oracle's reconstruction
        yt = R.reconstruct_torch(S.real.T, S.imag.T, torch.as_tensor(m), N, hop, n_out).numpy()
        assert np.max(np.abs(yt - y)) <= 1e-12 * max(np.max(np.abs(y)), 1e-300)


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_gradients_match_autograd_of_the_definitions(kind):
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 4097):
        for scale, noise in ((0.3, 0.3), (0.3, 0.01), (1e-3, 1e-3)):
            s = scale * rng.standard_normal(n)
            a = s + noise * rng.standard_normal(n)
            loss, counted, g = R.wave_loss(a, s, kind)
            assert counted
            at = torch.tensor(a, requires_grad=True)
            lt = R.wave_loss_torch(at, torch.as_tensor(s), kind)
            lt.backward()
            assert abs(loss - float(lt.detach())) <= 1e-12 * max(abs(float(lt.detach())), 1.0)
            ga = at.grad.numpy()
            assert np.max(np.abs(g - ga)) <= 1e-9 * max(np.max(np.abs(ga)), 1e-300), (n, scale, noise)


def test_silent_reference_row_is_not_counted():
    a = np.random.default_rng(0).standard_normal(50)
    loss, counted, g = R.wave_loss(a, np.zeros(50), "si_sdr")
    assert loss == 0.0 and not counted and np.all(g == 0.0) and g.shape == (50,)
    loss, counted, g = R.wave_loss(a, np.zeros(50), "wave_mse")          # the MSE counts it
    assert counted and loss == float(np.mean(a * a)) and np.array_equal(g, 2.0 / 50 * a)
    assert R.wave_loss(np.zeros(0), np.zeros(0), "wave_mse")[:2] == (0.0, False)


def test_head_references_agree_with_the_fused_heads_references():
    """The cotangent form fed the MSE's own d_mask is the fused heads' reference gradient."""
    import drnmf_train_ref as DR
    import lstm_train_ref as LT
    rng = np.random.default_rng(8)
    rows, r, F = 11, 3, 9
    hidden, kc, kn = rng.random((rows, 2 * r)), 0.3 * rng.standard_normal((r, F)), 0.3 * rng.standard_normal((r, F))
    x, y, w = rng.random((rows, F)), rng.random((rows, F)), (rng.random(rows) < 0.7).astype(np.float64)
    for square in (False, True):
        _, _, dh, dkc, dkn = DR.head_loss_and_grads(x, hidden, kc, kn, y, w, square)
        mask = DR.head_forward_ref(hidden, kc, kn, square)[0]
        got = R.head_cot_grads(hidden, kc, kn, w[:, None] * (2.0 / F) * (x * mask - y) * x, square)
        for a, b in zip(got, (dh, dkc, dkn)):
            assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b))
    B, T, H = 2, 3, 5
    hid, wo, bo = rng.standard_normal((B, T, H)), rng.standard_normal((H, F)), rng.standard_normal(F)
    xm, yy, ww = rng.random((B, T, F)), rng.random((B, T, F)), np.ones((B, T))
    _, _, dh, dwo, dbo = LT.head_loss_and_grads(xm, hid, yy, ww, wo, bo)
    s = 1.0 / (1.0 + np.exp(-(hid @ wo + bo)))
    got = R.lstm_head_cot_grads(hid, wo, bo, ww[..., None] * (2.0 / F) * (xm * s - yy) * xm)
    for a, b in zip(got, (dh, dwo, dbo)):
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b))


# ---- the C ABI ----------------------------------------------------------------------------------------------------
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return set(re.findall(r"\b(drnmf_[a-z0-9_]+)\s*\(", src))


def test_header_is_plain_c_and_matches_the_binding(capi, tmp_path):
    declared = _declared()
    assert declared == NAMES
    assert declared == set(capi.WAVELOSS_SIGNATURES), declared ^ set(capi.WAVELOSS_SIGNATURES)
    for t in dir(capi):
        if t.endswith("SIGNATURES") and t != "WAVELOSS_SIGNATURES":
            assert not (declared & set(getattr(capi, t))), t
    L = capi.lib()
    for name in sorted(declared):
        assert getattr(L, name).argtypes == capi.WAVELOSS_SIGNATURES[name][1]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in declared:
        assert name in doc, name
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "no C compiler"
    src = tmp_path / "waveloss_header_check.c"
    src.write_text('#include "drnmf_waveloss.h"\ntypedef void (*fn_t)(void);\nstatic const fn_t refs[] = {\n' +
                   "".join("    (fn_t)%s,\n" % n for n in sorted(declared)) +
                   "};\nint main(void) { return refs[0] != 0 && DRNMF_WAVE_LOSS_BLOCK == %d && "
                   "DRNMF_WAVE_LOSS_MSE == %d && DRNMF_WAVE_LOSS_SI_SDR == %d ? 0 : 1; }\n"
                   % (capi.WAVE_LOSS_BLOCK, capi.WAVE_LOSSES["wave_mse"], capi.WAVE_LOSSES["si_sdr"]))
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_wave_loss_workspace_bytes(capi):
    L = capi.lib()
    for n_sig, ld in ((0, 100), (-1, 100), (3, 0), (3, -5)):
        assert L.drnmf_wave_loss_workspace_bytes(n_sig, ld) == 0
    for n_sig, ld in ((1, 1), (1, 4096), (1, 4097), (5, 10000), (512, 96000)):
        b = L.drnmf_wave_loss_workspace_bytes(n_sig, ld)
        assert b % 256 == 0 and b >= 32 * n_sig * -(-ld // 4096) + 8 * n_sig, (n_sig, ld, b)


def test_entry_points_validate_without_a_gpu(capi):
    """On a drnmf_create_unbound handle, with pointers that are never dereferenced: bad shapes, bad sizes and NULLs
    give DRNMF_ERR_INVALID_ARG (-1) with the entry's name, a short or NULL workspace DRNMF_ERR_WORKSPACE (-4),
    operand_f16 = 1 DRNMF_ERR_UNSUPPORTED (-2); of two faults the earlier check of the documented order wins; a
    valid call stops only at the missing device."""
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0

    def err():
        return L.drnmf_last_error(h)

    try:
        fake = ctypes.c_void_p(0x100000)

        # drnmf_istft_ragged_vjp: shape, N, NULL, ld_dm
        def vjp(handle=h, n_sig=3, b=2, T=9, N=64, hop=16, ln=fake, idx=fake, re_=fake, im=fake, g=fake, ld_g=100,
                crop=1, dm=fake, ld_dm=33):
            return L.drnmf_istft_ragged_vjp(handle, n_sig, b, T, N, hop, ln, idx, re_, im, g, ld_g, crop, dm, ld_dm,
                                            None)
        assert vjp(handle=None) == -1
        for kw in (dict(n_sig=0), dict(b=0), dict(b=65536), dict(T=0), dict(hop=0), dict(ld_g=0), dict(crop=2),
                   dict(crop=-1)):
            assert vjp(**kw) == -1 and b"istft_ragged_vjp: bad shape" in err(), kw
        for N in (0, 32, 96, 8192):
            assert vjp(N=N, ld_dm=N // 2 + 1) == -1 and b"power of two in [64,4096]" in err(), N
        for name in ("ln", "idx", "re_", "im", "g", "dm"):
            assert vjp(**{name: None}) == -1 and b"istft_ragged_vjp: NULL" in err(), name
        assert vjp(ld_dm=32) == -1 and b"ld_dm=32 is below N/2+1=33" in err()
        assert vjp(T=0, N=96) == -1 and b"bad shape" in err()              # shape before N
        assert vjp(N=96, g=None) == -1 and b"power of two" in err()        # N before NULL
        assert vjp(g=None, ld_dm=1) == -1 and b"NULL" in err()             # NULL before ld_dm
        assert vjp() not in (0, -1, -2, -4)

        # drnmf_wave_loss: shape, kind, NULL, workspace
        need = L.drnmf_wave_loss_workspace_bytes(3, 5000)

        def loss(handle=h, n_sig=3, ld=5000, ln=fake, est=fake, ref=fake, kind=1, lo=fake, co=fake, g=fake, sums=fake,
                 ws=fake, ws_bytes=need):
            return L.drnmf_wave_loss(handle, n_sig, ld, ln, est, ref, kind, lo, co, g, sums, ws, ws_bytes, None)
        assert loss(handle=None) == -1
        for kw in (dict(n_sig=0), dict(n_sig=-2), dict(ld=0), dict(ld=-7), dict(n_sig=2 ** 31 - 1, ld=2 ** 40)):
            assert loss(**kw) == -1 and b"wave_loss: bad shape" in err(), kw
        for kind in (-1, 2):
            assert loss(kind=kind) == -1 and b"wave_loss: kind=" in err()
        for name in ("ln", "est", "ref", "lo", "co", "g", "sums"):
            assert loss(**{name: None}) == -1 and b"wave_loss: NULL" in err(), name
        for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
            assert loss(**kw) == -4 and b"wave_loss: workspace" in err(), kw
        assert loss(ld=0, kind=7) == -1 and b"bad shape" in err()          # shape before kind
        assert loss(kind=7, est=None) == -1 and b"kind=" in err()          # kind before NULL
        assert loss(est=None, ws=None) == -1 and b"NULL" in err()          # NULL before workspace
        for kind in (0, 1):
            assert loss(kind=kind) not in (0, -1, -2, -4) and b"no device" in err()

        # drnmf_head_backward_cot: shape (ld_dm included), NULL, workspace
        hneed = L.drnmf_loss_head_workspace_bytes(40, 33, 4)

        def head(handle=h, rows=40, F=33, r=4, hid=fake, ld_h=8, h_off=0, kc=fake, kn=fake, square=0, A=fake, Bn=fake,
                 dm=fake, ld_dm=33, dh=fake, dkc=fake, dkn=fake, ws=fake, ws_bytes=hneed):
            return L.drnmf_head_backward_cot(handle, rows, F, r, hid, ld_h, h_off, kc, kn, square, A, Bn, dm, ld_dm,
                                             dh, dkc, dkn, ws, ws_bytes, None)
        assert head(handle=None) == -1
        for kw in (dict(rows=0), dict(F=0), dict(r=0), dict(h_off=-1), dict(ld_h=7), dict(h_off=1), dict(ld_dm=32)):
            assert head(**kw) == -1 and b"head_backward_cot: bad shape" in err(), kw
        for name in ("hid", "kc", "kn", "A", "Bn", "dm", "dh", "dkc", "dkn", "ws"):
            assert head(**{name: None}) == -1 and b"head_backward_cot: NULL" in err(), name
        for kw in (dict(ws_bytes=hneed - 1), dict(ws_bytes=0)):
            assert head(**kw) == -4 and b"head_backward_cot: workspace" in err(), kw
        assert head(rows=0, dm=None) == -1 and b"bad shape" in err()       # shape before NULL
        assert head(dm=None, ws_bytes=0) == -1 and b"NULL" in err()        # NULL before workspace
        for square in (0, 1):
            assert head(square=square) not in (0, -1, -2, -4)

        # drnmf_lstm_head_backward_cot: the descriptor, operand_f16, workspace, NULL, ld_h / params, ld_dm
        d = capi.LstmDesc(3, 5, 9, 13, 2, capi.ACTIVATIONS["hard_sigmoid"], 0)
        lneed = L.drnmf_lstm_train_workspace_bytes(ctypes.byref(d))
        ws = ctypes.c_void_p(0x100000)

        def lstm(handle=h, desc=d, dm=fake, ld_dm=9, hid=fake, ld_h=16, params=ws, wo=fake, dh=fake, dwo=fake, dbo=fake,
                 w=ws, w_bytes=lneed):
            return L.drnmf_lstm_head_backward_cot(handle, ctypes.byref(desc) if desc is not None else None, dm, ld_dm,
                                                  hid, ld_h, params, wo, dh, dwo, dbo, w, w_bytes, None)
        assert lstm(handle=None) == -1
        d16 = capi.LstmDesc(3, 5, 9, 13, 2, capi.ACTIVATIONS["hard_sigmoid"], 1)
        assert lstm(desc=d16) == -2 and b"lstm_head_backward_cot: operand_f16 = 1 is inference only" in err()
        assert lstm(desc=d16, dm=None, w_bytes=0) == -2                    # the refusal before NULL and workspace
        assert lstm(desc=capi.LstmDesc(0, 5, 9, 13, 2, 5, 0)) == -1
        assert lstm(w=None) == -1 and b"lstm_head_backward_cot: NULL workspace" in err()
        assert lstm(w_bytes=lneed - 1) == -4 and b"lstm_head_backward_cot: workspace" in err()
        for name in ("dm", "hid", "params", "wo", "dh", "dwo", "dbo"):
            assert lstm(**{name: None}) == -1 and b"lstm_head_backward_cot: NULL pointer" in err(), name
        assert lstm(ld_h=12) == -1 and b"lstm_head_backward_cot: ld_h 12 < H 13" in err()
        assert lstm(ld_dm=8) == -1 and b"lstm_head_backward_cot: ld_dm 8 < F 9" in err()
        assert lstm(w_bytes=0, dm=None) == -4                              # workspace before NULL
        assert lstm(dm=None, ld_dm=1) == -1 and b"NULL pointer" in err()   # NULL before ld_dm
        assert lstm(ld_h=12, ld_dm=1) == -1 and b"ld_h 12" in err()        # ld_h before ld_dm
        assert lstm() not in (0, -1, -2, -4)
    finally:
        L.drnmf_destroy(h)


def test_ops_refuse_before_the_device_is_touched(capi):
    from drnmf_amd import ops
    a = torch.zeros((2, 9, 33))
    with pytest.raises(ValueError, match="no CPU"):
        ops.wave_loss(torch.zeros((2, 10)), torch.zeros((2, 10)), [10, 10])
    with pytest.raises(ValueError, match="loss must be one of"):
        ops.wave_loss(torch.zeros((2, 10)), torch.zeros((2, 10)), [10, 10], loss="sdr")
    with pytest.raises(ValueError, match="est, ref"):
        ops.wave_loss(torch.zeros((2, 10)), torch.zeros((2, 11)), [10, 10])
    with pytest.raises(ValueError, match="re, im must be"):
        ops.istft_ragged_vjp(torch.zeros((2, 100)), a, a[:, :, :32], [50, 60], 64, 16)
    with pytest.raises(ValueError, match="no CPU"):
        ops.istft_ragged_vjp(torch.zeros((2, 100)), a, a, [50, 60], 64, 16)


def test_models_refuse_before_the_device_is_touched(capi):
    """These run on a machine without a GPU: every refusal of the waveform trainers comes before the first
    allocation."""
    from drnmf_amd import layers
    a, b = np.zeros(1000, np.float32), np.zeros(700, np.float32)

    class Fake(layers._SequenceModel):
        mask_value = -1.0

        def __init__(self, stateful=False, compiled=True):
            self._st = stateful
            if compiled:
                self._flat = None

        def _device(self):
            return "cuda:0"

        def _input_width(self):
            return 33

        def _stateful(self):
            return self._st

    for call in ("train_on_wavs", "test_on_wavs", "fit_waveform"):
        with pytest.raises(NotImplementedError, match="stateful"):
            getattr(Fake(stateful=True), call)([a], [b], N=64, hop=16)
        with pytest.raises(ValueError, match="bins"):
            getattr(Fake(), call)([a], [b], N=128, hop=16)
        with pytest.raises(ValueError, match="loss must be one of"):
            getattr(Fake(), call)([a], [b], loss="sdr", N=64, hop=16)
        for bad in ([], [a, b], [a.astype(np.float64)], [np.zeros((2, 10), np.float32)], [np.zeros(0, np.float32)]):
            with pytest.raises(ValueError, match=call):
                getattr(Fake(), call)(bad, [a], N=64, hop=16)
        with pytest.raises(ValueError, match="max_samples"):
            getattr(Fake(), call)([a], [b], N=64, hop=16, max_samples=0)
    for call in ("train_on_wavs", "fit_waveform"):
        with pytest.raises(ValueError, match="compile"):
            getattr(Fake(compiled=False), call)([a], [b], N=64, hop=16)
    for call in ("train_on_batch_custom", "loss_and_grads_cot"):
        with pytest.raises(ValueError, match="compile"):
            getattr(Fake(compiled=False), call)(None, None)
        with pytest.raises(NotImplementedError, match="stateful"):
            getattr(Fake(stateful=True), call)(None, None)
    # the pieces: both sides clipped to the shorter, then cut at the same places
    rx, ry, dt = Fake._wave_pieces([a, b], [b, a], 64, 16, 300, "t")
    assert [v.shape[0] for v in rx] == [300, 300, 100] * 2 == [v.shape[0] for v in ry] and dt == np.float32
    model = layers.build_snmf(dict(r=4, sparsity=0.1, cf='ed', max_iter=2, conv_eps=0., random_seed=1),
                              np.ones((33, 8), np.float32), device="cpu")
    for call in ("train_on_wavs", "test_on_wavs", "fit_waveform"):
        with pytest.raises(NotImplementedError, match="SparseNMFModel"):
            getattr(model, call)([a], [b], N=64, hop=16)
    with pytest.raises(NotImplementedError, match="SparseNMFModel"):
        model.train_on_batch_custom(None, None)
