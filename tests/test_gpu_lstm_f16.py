"""The LSTM baseline with fp16 matrix-core operands on the GPU (operand_f16 of drnmf_lstm_desc_t, csrc/lstm.hip's
lstm_step_kernel<false, true>; LSTM(operand_dtype='float16')).

References (tests/lstm_f16_ref.py, shared with tests/test_lstm_f16_host.py, which establishes on the CPU that they
are far enough apart): the fp64 EMULATION of the mode -- operands of the recurrent products rounded to fp16,
everything else exact -- and the EXACT fp64 reference of the fp32 model.  On the head output, max|d| / max|ref|:
  tight  distance to the emulation <= TOL_EMU = 4 max(D_acc, D_f32): D_acc the recorded distance between two
         accumulation orders of the emulation, D_f32 = 1e-4 the fp32 kernels' tolerance, 4 for the device's own
         order.  The exact reference is at least 4 TOL_EMU away (host test), so an implementation that ignores the
         flag fails here.
  loose  distance to the exact reference <= 2 D_f16, D_f16 = the distance between the two references.
DRNMF_TEST_MATRIX_MODE=bf16x3: the input projection and the head follow the matrix mode.  Its error against fp64 is
within 2x the fp32 pipe's, 2e-6 at the worst (profiles/r06_x3_error_table.md), fifty times below D_f32: TOL_EMU
needs nothing added.
"""
import numpy as np
import pytest
import torch

import lstm_f16_ref as E
import lstm_state_ref as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (run with -m 'not gpu' on CPU boxes)")
    from drnmf_amd import _capi
    _capi.handle(0)
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)          # (a copy: the shared references are read-only)


def _prepare(dev, w, F, H, K, act):
    from drnmf_amd import ops
    t = lambda a: _t(a, dev)
    return ops.lstm_prepare_params(ops.make_lstm_desc(1, 1, F, H, K, act, operand_f16=True),
                                   [t(a) for a in w[0:3 * K:3]], [t(a) for a in w[1:3 * K:3]],
                                   [t(a) for a in w[2:3 * K:3]], t(w[-2]), t(w[-1]))


def _run(dev, params, x, F, H, K, act, state=None, final=None):
    """lstm_forward + lstm_head_forward with an fp16 descriptor -> (y, hidden) device tensors"""
    from drnmf_amd import ops
    x = x if isinstance(x, torch.Tensor) else _t(x, dev)
    desc = ops.make_lstm_desc(x.shape[0], x.shape[1], F, H, K, act, operand_f16=True)
    kw = {}
    if state is not None or final is not None:
        kw = dict(initial_state=state, final_state=final)
    h = ops.lstm_forward(x, -1.0, params, desc, **kw)
    return ops.lstm_head_forward(h, params, desc), h


def _check(got, ref, tol, what):
    err = E.rel(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, ref)
    print("%s: max|d|/max|ref| = %.3e (bound %.3e)" % (what, err, tol))
    assert err <= tol, "%s: max|d|/max|ref| = %.3e > %.3e" % (what, err, tol)


@pytest.mark.parametrize("i", range(len(E.CASES)), ids=[c.id for c in E.CASES])
def test_forward_matches_the_emulation(dev, i):
    from drnmf_amd import ops
    cs = E.CASES[i]
    B, T, F, H, K = cs.shape
    x, w, st, y_emu, h_emu, y_exact = E.case_data(i)
    params = _prepare(dev, w, F, H, K, cs.act)
    state = None if st is None else tuple(_t(s, dev) for s in st)
    y, h = _run(dev, params, x, F, H, K, cs.act, state)
    torch.cuda.synchronize()
    _check(y, y_emu, cs.tol_emu, "output vs emulation")
    _check(y, y_exact, 2 * E.rel(y_emu, y_exact), "output vs exact reference")
    ld = ops.lstm_hidden_ld(H)
    assert h.stride() == (T * ld, ld, 1)
    if ld > H:
        assert float(h.as_strided((B, T, ld), (T * ld, ld, 1))[..., H:].abs().max()) == 0.0
    if cs.inp == "ragged" and B > 1 and st is None:      # the all-masked row: zero states in every frame
        assert float(h[-1].abs().max()) == 0.0


def test_single_frame_from_the_zero_state(dev):
    """(1, 1, 5, 13, 1) as drnmf_lstm_forward runs it: the recurrent product meets the zero shadow state, the output
    is the emulation's (which here is the exact reference's)."""
    cs = E.CASES[0]
    B, T, F, H, K = cs.shape
    x, w, _, _, _, _ = E.case_data(0)
    y_emu, h_emu, _ = E.model_forward(x, w, K, -1.0, cs.act)
    y, h = _run(dev, _prepare(dev, w, F, H, K, cs.act), x, F, H, K, cs.act)
    _check(h, h_emu, cs.tol_emu, "hidden vs emulation")
    _check(y, y_emu, cs.tol_emu, "output vs emulation")


def test_two_cuts_equal_the_one_call_run(dev):
    """(4, 6, 17, 32, 2) cut into T = 4 and T = 2 through drnmf_lstm_forward_stateful, the state carried in place:
    h_out equals the one-call run bit for bit, as tests/test_gpu_lstm_state.py asks of the fp32 kernels -- the
    carried state is fp32 and the shadow is rounded from it again at the start of the second call.  The sigmoid
    outputs (head products of different row counts) within atol = 1e-6, as there."""
    i = len(E.CASES) - 1
    cs = E.CASES[i]
    B, T, F, H, K = cs.shape
    assert (B, T, F, H, K) == (4, 6, 17, 32, 2)
    x, w, _, y_emu, _, _ = E.case_data(i)
    params = _prepare(dev, w, F, H, K, cs.act)
    y_whole, h_whole = _run(dev, params, x, F, H, K, cs.act)
    st = tuple(torch.zeros((K, B, H), dtype=torch.float32, device=dev) for _ in range(2))
    y1, h1 = _run(dev, params, x[:, :4], F, H, K, cs.act, st, st)
    y2, h2 = _run(dev, params, x[:, 4:], F, H, K, cs.act, st, st)
    torch.cuda.synchronize()
    h_cut, y_cut = torch.cat([h1, h2], dim=1), torch.cat([y1, y2], dim=1)
    assert torch.equal(h_cut, h_whole), "cuts vs one call: max|d| = %.3e" % float((h_cut - h_whole).abs().max())
    np.testing.assert_allclose(y_cut.cpu().numpy(), y_whole.cpu().numpy(), rtol=0, atol=1e-6)


def test_nonzero_entering_state(dev):
    """The same shape from a non-zero (h, c): initial_h reaches the products through the shadow, rounded.  The
    fp32 state the call leaves is held to the emulation's by the tight bound's formula, 4 max(D_acc, D_f32), with
    D_acc taken on that state array from the emulation's two accumulation orders."""
    i = len(E.CASES) - 1
    cs = E.CASES[i]
    B, T, F, H, K = cs.shape
    x, w, _, y_zero, _, _ = E.case_data(i)
    st0 = SR.random_state(np.random.default_rng(5), K, B, H)
    y_emu, h_emu, fin = E.model_forward(x, w, K, -1.0, cs.act, "fp64", st0)
    assert E.rel(y_emu, y_zero) > 100 * cs.tol_emu           # the state matters
    st = tuple(_t(s, dev) for s in st0)
    y, h = _run(dev, _prepare(dev, w, F, H, K, cs.act), x, F, H, K, cs.act, st, st)
    torch.cuda.synchronize()
    _check(y, y_emu, cs.tol_emu, "output vs emulation")
    fin_chunk = E.model_forward(x, w, K, -1.0, cs.act, "fp32chunk", st0)[2]
    for got, ref, alt, name in zip(st, fin, fin_chunk, ("final_h", "final_c")):
        _check(got, ref, 4 * max(E.rel(alt, ref), E.D_F32), name + " vs emulation")


def _model(dev, F, H, K, act, dtype):
    from drnmf_amd import layers
    return layers.build_lstm(dict(mask_value=-1., maxseq=8, input_dim=F, output_dim=F, K_layers=K, hidden_dim=H,
                                  recurrent_activation=act, operand_dtype=dtype), device=dev)


def test_model_level(dev):
    from drnmf_amd import layers
    i = 2
    cs = E.CASES[i]
    B, T, F, H, K = cs.shape
    x, w, _, y_emu, _, _ = E.case_data(i)
    m32 = _model(dev, F, H, K, cs.act, "float32")
    m32.set_weights([np.array(a) for a in w])
    m = _model(dev, F, H, K, cs.act, "float16")
    m.set_weights(m32.get_weights())                     # float32 arrays from a float32 model
    for a in m.weights:
        assert a.dtype == torch.float32
    xd = _t(x, dev)
    y, h = m.forward(xd, want_hidden=True)
    y_ops, h_ops = _run(dev, _prepare(dev, w, F, H, K, cs.act), x, F, H, K, cs.act)
    torch.cuda.synchronize()
    assert torch.equal(h, h_ops) and torch.equal(y, y_ops)
    _check(y, y_emu, cs.tol_emu, "model output vs emulation")
    # the float32 model of the same weights is NOT within the tight bound of the emulation: the flag is live
    assert E.rel(m32.forward(xd).cpu().numpy(), y_emu) > cs.tol_emu
    # predict: slabs of 8 out of 17 ragged rows, length-sorted and trimmed, = forward row by row
    out = m.predict(np.array(x), batch_size=8)
    np.testing.assert_allclose(out, y.cpu().numpy(), rtol=0, atol=1e-6)
    with pytest.raises(NotImplementedError, match="float32"):
        m.compile(lr=1e-4)
    mixed = [layers.LSTM(H, return_sequences=True, device=dev, operand_dtype=dt) for dt in ("float32", "float16")]
    with pytest.raises(ValueError, match="operand_dtype"):
        layers.LSTMModel([], mixed, m.dense, -1., dev)
