"""CPU-side tests of the stateful LSTM baseline (no GPU needed): the fp64 reference with entering and leaving
state (tests/lstm_state_ref.py) against tests/lstm_ref.py on concatenated chunks, the size of the entering state's
share of the gradients (so that the GPU gradient test cannot pass on a kernel that ignores the state), the
argument validation of the *_stateful entry points, and the layer surface (LSTM(stateful=True), build_lstm,
LSTMModel)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import lstm_ref as R
import lstm_state_ref as SR
import lstm_train_ref as TR

G_TOL = 2e-3          # the gradient bound of test_gpu_lstm_train.py / test_gpu_lstm_state.py


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


@pytest.mark.parametrize("act", ["hard_sigmoid", "sigmoid"])
@pytest.mark.parametrize("K", [1, 3])
def test_chunked_reference_equals_lstm_ref_on_the_concatenation(K, act):
    """Chunks of lengths (1, 2, 5, 4) with the state carried = lstm_ref on the 12 frames at once: with masked
    prefixes, suffixes, interior runs and a fully masked row, so the masked-output rule (carried h, not zeros) is
    what makes the two agree."""
    rng = np.random.default_rng(20 + K)
    B, F, H = 7, 9, 10
    cuts = (1, 2, 5, 4)
    w = R.random_weights(rng, F, H, K, scale=1.5)
    x, _ = R.masked_input(rng, B, sum(cuts), F)
    y_ref, h_ref = R.model_forward(x, w, K, -1.0, act)
    y, h, (fh, fc) = SR.chunked_forward(x, cuts, w, K, -1.0, act)
    assert np.abs(h - h_ref).max() <= 1e-13 and np.abs(y - y_ref).max() <= 1e-13
    assert np.abs(fh[-1] - h_ref[:, -1]).max() <= 1e-13
    # zero state spelled out = no state
    z = np.zeros((K, B, H))
    y0, h0, _ = SR.model_forward(x, w, K, -1.0, act, state=(z, z))
    assert np.array_equal(y0, y_ref) and np.array_equal(h0, h_ref)


def test_reference_masked_rows_keep_their_state_and_output():
    rng = np.random.default_rng(3)
    B, T, F, H, K = 3, 5, 6, 4, 2
    w = R.random_weights(rng, F, H, K, scale=1.5)
    x = rng.random((B, T, F)).astype(np.float32)
    x[1] = -1.0                                    # masked for the whole call
    x[2, :2] = -1.0                                # masked prefix
    st = SR.random_state(rng, K, B, H)
    _, h, (fh, fc) = SR.model_forward(x, w, K, -1.0, "hard_sigmoid", state=st)
    assert np.array_equal(fh[:, 1], st[0][:, 1].astype(np.float64))
    assert np.array_equal(fc[:, 1], st[1][:, 1].astype(np.float64))
    for t in range(T):
        assert np.array_equal(h[1, t], st[0][-1, 1].astype(np.float64))
    assert np.array_equal(h[2, 0], st[0][-1, 2].astype(np.float64))
    assert np.array_equal(h[2, 1], st[0][-1, 2].astype(np.float64))


def test_entering_state_moves_the_gradients_by_far_more_than_the_bound():
    """Must-fail-without-the-feature guard of the GPU gradient test: at its first shape, with an entering state of
    magnitude about 1, the reference's recurrent-kernel gradients and the f-gate columns of its kernel gradients
    differ from the zero-state ones by more than 10 * G_TOL (max|d| / max|ref|) -- a BPTT that ignored the entering
    h or c could not pass the GPU test.  With the zero state the reference equals lstm_train_ref."""
    B, T, F, H, K = 3, 6, 9, 10, 2
    rng = np.random.default_rng(41)
    w = R.random_weights(rng, F, H, K, scale=1.5)
    x = rng.random((B, T, F)).astype(np.float32)
    y = rng.random((B, T, F)).astype(np.float32)
    sw = np.ones((B, T), np.float32)
    st = SR.random_state(rng, K, B, H)
    l0, c0, g0, _ = SR.loss_and_grads(x, y, sw, w, K)
    l1, c1, g1, _ = SR.loss_and_grads(x, y, sw, w, K, state=st)
    lr, cr, gr = TR.loss_and_grads(x, y, sw, w, K)
    assert l0 == lr and c0 == cr and all(np.array_equal(a, b) for a, b in zip(g0, gr))
    rel = lambda a, b: float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-30)
    for k in range(K):
        assert rel(g0[3 * k + 1], g1[3 * k + 1]) > 10 * G_TOL, "recurrent_kernel %d" % k
        assert rel(g0[3 * k][:, H:2 * H], g1[3 * k][:, H:2 * H]) > 10 * G_TOL, "kernel %d, f columns" % k
    assert abs(l0 - l1) > 1e-3 * abs(l1)


def test_stateful_entry_points_validate_without_a_gpu(capi):
    """drnmf_create_unbound handle: the new entry points refuse NULL required pointers, a bad ld_h and short
    workspaces with the codes of the existing ones (-1 DRNMF_ERR_INVALID_ARG, -4 DRNMF_ERR_WORKSPACE); the state
    pointers themselves may be NULL."""
    from drnmf_amd import ops
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)          # never dereferenced: validation fails first
        good = ops.make_lstm_desc(4, 10, 33, 13, 2)
        for fn, need in ((L.drnmf_lstm_forward_stateful, L.drnmf_lstm_workspace_bytes(ctypes.byref(good))),
                         (L.drnmf_lstm_train_forward_stateful,
                          L.drnmf_lstm_train_workspace_bytes(ctypes.byref(good)))):
            call = lambda d=good, x=fake, p=fake, out=fake, ld=16, ws=fake, n=need, st=(fake,) * 4, hh=h: \
                fn(hh, ctypes.byref(d) if d is not None else None, x, -1.0, p, st[0], st[1], st[2], st[3], out, ld,
                   ws, n, None)
            for field, v in (("B", 0), ("T", -1), ("F", 0), ("H", 0), ("K", 0), ("recurrent_activation", 99)):
                d = ops.make_lstm_desc(4, 10, 33, 13, 2)
                setattr(d, field, v)
                assert call(d=d) == -1
            assert call(d=None) == -1
            assert call(hh=None) == -1
            assert call(x=None) == -1 and call(p=None) == -1 and call(out=None) == -1 and call(ws=None) == -1
            assert call(ld=12) == -1                     # row stride ld_h < H
            assert call(n=need - 1) == -4
            assert b"workspace" in L.drnmf_last_error(h)
            assert call(n=need - 1, st=(None,) * 4) == -4    # NULL state pointers are not what is refused
    finally:
        L.drnmf_destroy(h)


def _params(K=2, H=13, F=20, **kw):
    return dict(mask_value=-1., maxseq=10, input_dim=F, output_dim=F, K_layers=K, hidden_dim=H, **kw)


def test_stateful_layer_surface():
    from drnmf_amd import layers, ops
    l = layers.LSTM(5, return_sequences=True, stateful=True, device="cpu")
    assert l.stateful is True
    assert layers.LSTM(5, return_sequences=True, device="cpu").stateful is False
    m = layers.build_lstm(_params(), device="cpu")
    assert not m._stateful() and all(not x.stateful for x in m.lstms)
    with pytest.raises(AttributeError):
        m.reset_states()
    ms = layers.build_lstm(_params(stateful=True), device="cpu")
    assert ms._stateful() and all(x.stateful for x in ms.lstms)
    assert [type(a).__name__ for a in ms.layers] == [type(a).__name__ for a in m.layers]
    ms.reset_states()                                # before the first call: nothing to zero
    assert ms._states is None
    # the states: [K,B,H] zeros on first use, bound to their batch size
    hs, cs = ms._state(4)
    assert tuple(hs.shape) == tuple(cs.shape) == (2, 4, 13) and not hs.any() and not cs.any()
    assert ms._state(4)[0] is hs
    with pytest.raises(ValueError):
        ms._state(5)
    hs.fill_(1.0)
    ms.reset_states()
    assert ms._state(4)[0] is hs and not hs.any()
    ms.reset_states(batch_size=5)
    assert tuple(ms._state(5)[0].shape) == (2, 5, 13)
    with pytest.raises(NotImplementedError):         # enhance stays closed to a stateful model
        ms.enhance([np.zeros(2048, np.int16)], N=38, hop=19)
    # the ops take the state keyword-only
    for fn in (ops.lstm_forward, ops.lstm_train_forward):
        sig = inspect.signature(fn)
        for n in ("initial_state", "final_state"):
            assert sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[n].default is None


def test_mixed_stateful_stack_is_refused():
    from drnmf_amd import layers
    m = layers.build_lstm(_params(K=3), device="cpu")
    lstms = list(m.lstms)
    odd = layers.LSTM(13, return_sequences=True, stateful=True, device="cpu")
    odd.build((None, 10, 13))
    with pytest.raises(ValueError):
        layers.LSTMModel(m.layers, [lstms[0], odd, lstms[2]], m.dense, -1.0, torch.device("cpu"))
    every = []
    for _ in range(3):
        l = layers.LSTM(13, return_sequences=True, stateful=True, device="cpu")
        l.build((None, 10, 13))
        every.append(l)
    assert layers.LSTMModel(m.layers, every, m.dense, -1.0, torch.device("cpu"))._stateful()
