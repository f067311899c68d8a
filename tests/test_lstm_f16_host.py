"""operand_f16 of the LSTM baseline without a GPU: the descriptor field and its validation, the sizes of the fp16
layouts, the refusal of the training entry points, the model-level plumbing, and the REFERENCE CONDITIONS of
tests/test_gpu_lstm_f16.py -- that its two references (the fp16-operand emulation and the exact fp64 reference)
are far enough apart, at each of its shapes, for the tight check to tell them apart."""
import ctypes

import numpy as np
import pytest

import lstm_f16_ref as E
import lstm_ref as R


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


def _up(v, m):
    return (v + m - 1) // m * m


def test_descriptor_field():
    from drnmf_amd import ops
    d = ops.make_lstm_desc(4, 10, 33, 13, 2, operand_f16=True)
    assert d.operand_f16 == 1
    assert (d.B, d.T, d.F, d.H, d.K) == (4, 10, 33, 13, 2)
    assert ops.make_lstm_desc(4, 10, 33, 13, 2).operand_f16 == 0
    assert ops.make_lstm_desc(4, 10, 33, 13, 2, "sigmoid").operand_f16 == 0
    assert ctypes.sizeof(d) == 7 * 4                      # seven int32, operand_f16 the last


def test_operand_f16_is_validated_and_training_refused(capi):
    """As tests/test_lstm_host.py reaches the other fields: entry points on an unbound handle, fake pointers that
    validation never dereferences."""
    from drnmf_amd import ops
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)
        ptrs = (ctypes.c_void_p * 2)(0x100000, 0x100000)
        good = ops.make_lstm_desc(4, 10, 33, 13, 2, operand_f16=True)
        need = L.drnmf_lstm_workspace_bytes(ctypes.byref(good))
        pneed = L.drnmf_lstm_params_bytes(ctypes.byref(good))
        for v in (2, -1):
            d = ops.make_lstm_desc(4, 10, 33, 13, 2)
            d.operand_f16 = v
            rc = L.drnmf_lstm_forward(h, ctypes.byref(d), fake, -1.0, fake, fake, 16, fake, need, None)
            assert rc == -1, rc                                                      # DRNMF_ERR_INVALID_ARG
            assert b"operand_f16" in L.drnmf_last_error(h)
            assert L.drnmf_lstm_forward_stateful(h, ctypes.byref(d), fake, -1.0, fake, None, None, None, None, fake,
                                                 16, fake, need, None) == -1
            assert L.drnmf_lstm_head_forward(h, ctypes.byref(d), fake, 16, fake, fake, None) == -1
            assert L.drnmf_lstm_prepare_params(h, ctypes.byref(d), fake, fake, fake, fake, fake, fake, fake, pneed,
                                               None) == -1
        g = ctypes.byref(good)
        # a good fp16 descriptor passes validation: the short workspace is what stops the call
        assert L.drnmf_lstm_forward(h, g, fake, -1.0, fake, fake, 16, fake, need - 1, None) == -4
        # training: size 0 and DRNMF_ERR_UNSUPPORTED from every entry point, the message naming the field
        assert L.drnmf_lstm_train_workspace_bytes(g) == 0
        big = 1 << 30
        calls = [
            lambda: L.drnmf_lstm_train_forward(h, g, fake, -1.0, fake, fake, 16, fake, big, None),
            lambda: L.drnmf_lstm_train_forward_stateful(h, g, fake, -1.0, fake, None, None, None, None, fake, 16,
                                                        fake, big, None),
            lambda: L.drnmf_lstm_loss_head_backward(h, g, fake, fake, fake, 16, fake, fake, fake, fake, fake, fake,
                                                    fake, big, None),
            lambda: L.drnmf_lstm_backward(h, g, ptrs, ptrs, fake, ptrs, ptrs, ptrs, fake, big, None),
        ]
        for call in calls:
            assert call() == -2                                                      # DRNMF_ERR_UNSUPPORTED
            assert b"operand_f16" in L.drnmf_last_error(h)
    finally:
        L.drnmf_destroy(h)


def _params_bytes(F, H, K, half):
    """The params layout of csrc/lstm.hip (lstm_layout), every block rounded up to 256 bytes:
      stacked matrices  (2 K - 1) Hc NC elements of 4 bytes (fp32) or 2 (fp16): recurrent_0 has Hc rows, every
                        [kernel_k; recurrent_k] 2 Hc; Hc = round_up(H, 16) (fp32) or round_up(H, 32) (fp16),
                        NC = 32 ceil(H / 8) packed gate columns
      bias K NC, kernel_0^T NC round_up(F, 4), W_out^T F round_up(H, 4), b_out F   -- fp32 in both modes"""
    Hc, NC = _up(H, 32 if half else 16), 32 * ((H + 7) // 8)
    blocks = [(2 * K - 1) * Hc * NC * (2 if half else 4), K * NC * 4, NC * _up(F, 4) * 4, F * _up(H, 4) * 4, F * 4]
    return sum(_up(b, 256) for b in blocks)


def test_params_and_workspace_sizes(capi):
    from drnmf_amd import ops
    L = capi.lib()
    pb = lambda d: L.drnmf_lstm_params_bytes(ctypes.byref(d))
    wb = lambda d: L.drnmf_lstm_workspace_bytes(ctypes.byref(d))
    F, H, K = 513, 250, 5
    d32, d16 = ops.make_lstm_desc(32, 50, F, H, K), ops.make_lstm_desc(32, 50, F, H, K, operand_f16=True)
    assert pb(d32) == _params_bytes(F, H, K, False) and pb(d16) == _params_bytes(F, H, K, True)
    assert pb(d16) < pb(d32)
    # H = 250: Hc = 256 in both modes, so the difference is exactly half of the stacked matrices
    assert pb(d32) - pb(d16) == (2 * K - 1) * 256 * (32 * 32) * 2
    # ... and at equal Hc the workspace grows by the fp16 shadow of the h ring, [K][2][Bp][Hc] halves
    assert wb(d16) - wb(d32) == _up(K * 2 * 32 * 256 * 2, 256)
    # Hc = round_up(H, 32): sizes at H = 13, 54, 70 are those of Hc = 32, 64, 96
    for Hh, Hc in ((13, 32), (54, 64), (70, 96)):
        B, T, Ff, Kk = 5, 7, 33, 3
        d = ops.make_lstm_desc(B, T, Ff, Hh, Kk, operand_f16=True)
        assert pb(d) == _params_bytes(Ff, Hh, Kk, True)
        NC, Bp, rows = 32 * ((Hh + 7) // 8), 16, B * T
        ws = [rows * _up(Ff, 4) * 4, rows, rows * NC * 4, Kk * 2 * Bp * Hc * 4, Kk * 2 * Bp * Hc * 4,
              Kk * 2 * Bp * Hc * 2, 256]
        assert wb(d) == sum(_up(b, 256) for b in ws), (Hh, Hc)


def _model_params(**kw):
    p = dict(mask_value=-1., maxseq=8, input_dim=7, output_dim=7, K_layers=2, hidden_dim=5)
    p.update(kw)
    return p


def test_model_plumbing_on_the_cpu():
    from drnmf_amd import layers
    m = layers.build_lstm(_model_params(operand_dtype="float16"), device="cpu")
    assert all(l.operand_dtype == "float16" for l in m.lstms)
    assert m._desc(3, 4).operand_f16 == 1
    m32 = layers.build_lstm(_model_params(), device="cpu")
    assert all(l.operand_dtype == "float32" for l in m32.lstms) and m32._desc(3, 4).operand_f16 == 0
    with pytest.raises(ValueError):
        layers.build_lstm(_model_params(operand_dtype="bfloat16"), device="cpu")
    with pytest.raises(ValueError):
        layers.LSTM(5, return_sequences=True, operand_dtype="float64")
    with pytest.raises(NotImplementedError, match="float32"):
        m.compile(lr=1e-4)
    # weights stay float32 arrays; a float32 model's weights go into a float16 model unchanged
    w = m32.get_weights()
    m.set_weights(w)
    for a, b in zip(w, m.get_weights()):
        assert b.dtype == np.float32 and a.tobytes() == b.tobytes()
    # a stack whose layers disagree is refused (as for stateful)
    mixed = [layers.LSTM(5, return_sequences=True, device="cpu", operand_dtype=dt) for dt in ("float16", "float32")]
    with pytest.raises(ValueError, match="operand_dtype"):
        layers.LSTMModel([], mixed, m.dense, -1., m.device)


def test_emulation_without_rounding_is_the_reference(monkeypatch):
    """The emulation differs from lstm_ref only in the rounding: with f16() the identity it reproduces it."""
    rng = np.random.default_rng(0)
    B, T, F, H, K = 4, 6, 9, 10, 3
    w = R.random_weights(rng, F, H, K, scale=2.0)
    x, _ = R.masked_input(rng, B, T, F)
    monkeypatch.setattr(E, "f16", lambda a: np.asarray(a, dtype=np.float64))
    for act in ("hard_sigmoid", "sigmoid"):
        y, h, _ = E.model_forward(x, w, K, -1.0, act)
        y_ref, h_ref = R.model_forward(x, w, K, -1.0, act)
        assert np.max(np.abs(h - h_ref)) <= 1e-13 and np.max(np.abs(y - y_ref)) <= 1e-13


@pytest.mark.parametrize("i", range(len(E.CASES)), ids=[c.id for c in E.CASES])
def test_reference_conditions(i):
    """On the head output, max|d| / max|ref|:
      D_acc  fp64-accumulate emulation vs fp32-chunk-accumulate emulation (under the recorded constant)
      D_f16  fp64-accumulate emulation vs the exact reference
      D_f32  the TOL tests/test_gpu_lstm.py holds the fp32 kernels to
    and 4 max(D_acc, D_f32) <= D_f16 / 4: the exact reference -- hence any implementation that ignores the flag --
    is at least four times the tight bound TOL_EMU away from the emulation, and the emulation is inside a quarter
    of the loose bound 2 D_f16."""
    cs = E.CASES[i]
    x, w, st, y_emu, _, y_exact = E.case_data(i)
    y_chunk, _, _ = E.model_forward(x, w, cs.shape[4], -1.0, cs.act, "fp32chunk", st)
    d_acc, d_f16 = E.rel(y_chunk, y_emu), E.rel(y_emu, y_exact)
    print("%s: D_acc = %.3e, D_f16 = %.3e" % (cs.id, d_acc, d_f16))
    assert d_acc <= cs.d_acc
    assert cs.tol_emu == 4 * max(cs.d_acc, E.D_F32)
    assert 4 * max(cs.d_acc, E.D_F32) <= d_f16 / 4
