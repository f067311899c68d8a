"""The stateful LSTM baseline on the GPU (drnmf_lstm_forward_stateful / drnmf_lstm_train_forward_stateful in
csrc/lstm.hip, LSTMModel(stateful)): h and c carried across calls.

Forward oracle: chunks run with the state carried must equal tests/lstm_ref.py on the concatenated frames,
max|d| / max|ref| <= 1e-4 (TOL of test_gpu_lstm.py), and the one-call GPU run of the same frames bit for bit on
h_out (the recurrence is a fixed-order computation per (layer, frame), and the input projection's rows do not
depend on the row count at these shapes).  Training: tests/lstm_state_ref.py's fp64 autograd with a detached
entering state, loss within L_TOL = 1e-5 relative and every weight array's gradient within G_TOL = 2e-3
(max|d| / max|ref|), the bounds of test_gpu_lstm_train.py; tests/test_lstm_state_host.py shows on the CPU that
the entering state moves those gradients by more than 10 G_TOL.  Sigmoid outputs of runs whose head product has
different row counts are compared with atol = 1e-6, as test_predict_slabs_and_length_aware_run does.
"""
import numpy as np
import pytest
import torch

import lstm_ref as R
import lstm_state_ref as SR

pytestmark = pytest.mark.gpu

TOL = 1e-4
G_TOL = 2e-3
L_TOL = 1e-5
CUTS = (1, 2, 5, 4)          # T odd and even: the leaving state sits in ring slot 0 and in slot 1; T = 1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (run with -m 'not gpu' on CPU boxes)")
    from drnmf_amd import _capi
    _capi.handle(0)
    return torch.device("cuda:0")


def _rel(got, ref):
    return float(np.max(np.abs(got - ref))) / max(float(np.max(np.abs(ref))), 1e-30)


def _check(got, ref, what, tol=TOL):
    err = _rel(got, ref)
    assert err <= tol, "%s: max|d|/max|ref| = %.3e" % (what, err)


class Net(object):
    """Weights + prepared block of one (F, H, K, activation); run() = one C-ABI call on a chunk."""

    def __init__(self, dev, F, H, K, act="hard_sigmoid", seed=0, scale=1.5):
        from drnmf_amd import ops
        self.dev, self.F, self.H, self.K, self.act = dev, F, H, K, act
        self.w = R.random_weights(np.random.default_rng(seed), F, H, K, scale=scale)
        t = lambda a: torch.from_numpy(a).to(dev)
        w = self.w
        self.params = ops.lstm_prepare_params(ops.make_lstm_desc(1, 1, F, H, K, act), [t(a) for a in w[0:3 * K:3]],
                                              [t(a) for a in w[1:3 * K:3]], [t(a) for a in w[2:3 * K:3]],
                                              t(w[-2]), t(w[-1]))

    def state(self, B, value=None):
        if value is None:
            return tuple(torch.zeros((self.K, B, self.H), dtype=torch.float32, device=self.dev) for _ in range(2))
        return tuple(torch.from_numpy(np.ascontiguousarray(v)).to(self.dev) for v in value)

    def run(self, x, train=False, **kw):
        from drnmf_amd import ops
        x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)
        desc = ops.make_lstm_desc(x.shape[0], x.shape[1], self.F, self.H, self.K, self.act)
        if train:
            return ops.lstm_train_forward(x, -1.0, self.params, desc, ops.lstm_train_workspace(desc, self.dev), **kw)
        return ops.lstm_forward(x, -1.0, self.params, desc, **kw)

    def chunks(self, x, cuts, st, train=False):
        """Chunks with `st` carried in place (final aliased to initial) -> h_out of all frames, and the state
        after every chunk (host copies)."""
        hs, states, t0 = [], [], 0
        for n in cuts:
            hs.append(self.run(x[:, t0:t0 + n], train=train, initial_state=st, final_state=st))
            states.append(tuple(s.cpu().numpy() for s in st))
            t0 += n
        return torch.cat(hs, dim=1), states


def _ref_states(net, x, cuts, state=None):
    out, t0 = [], 0
    for n in cuts:
        _, _, state = SR.model_forward(x[:, t0:t0 + n], net.w, net.K, -1.0, net.act, state)
        out.append(state)
        t0 += n
    return out


# (B, F, H, K): rows B .. Bp-1 and units H .. Hc-1 are padding in both; K = 1, 2, 3
SHAPES = [(3, 9, 10, 2), (17, 33, 24, 3), (3, 9, 10, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%dF%dH%dK%d" % s)
def test_chunked_forward_equals_the_reference_and_the_one_call_run(dev, shape):
    B, F, H, K = shape
    rng = np.random.default_rng(B + H + K)
    net = Net(dev, F, H, K, seed=H + K)
    x, _ = R.masked_input(rng, B, sum(CUTS), F)
    h, states = net.chunks(x, CUTS, net.state(B))
    whole = net.run(x)
    torch.cuda.synchronize()
    _, h_ref = R.model_forward(x, net.w, K, -1.0, net.act)
    _check(h.cpu().numpy(), h_ref, "hidden, chunked")
    assert torch.equal(h, whole), "chunked vs one call: max|d| = %.3e" % float((h - whole).abs().max())
    for i, ((fh, fc), (rh, rc)) in enumerate(zip(states, _ref_states(net, x, CUTS))):
        _check(fh, rh, "final_h after chunk %d" % i)
        _check(fc, rc, "final_c after chunk %d" % i)


@pytest.mark.parametrize("act", ["hard_sigmoid", "sigmoid"])
def test_nonzero_entering_state_both_activations(dev, act):
    B, F, H, K = 3, 9, 10, 2
    rng = np.random.default_rng(7)
    net = Net(dev, F, H, K, act=act, seed=3)
    x, _ = R.masked_input(rng, B, 6, F)
    st0 = SR.random_state(rng, K, B, H)
    st = net.state(B, st0)
    h = net.run(x, initial_state=st, final_state=st)
    torch.cuda.synchronize()
    _, h_ref, (rh, rc) = SR.model_forward(x, net.w, K, -1.0, act, state=st0)
    _check(h.cpu().numpy(), h_ref, "hidden")
    _check(st[0].cpu().numpy(), rh, "final_h")
    _check(st[1].cpu().numpy(), rc, "final_c")
    # the zero-state answer is far away: the entering state is really used
    assert _rel(R.model_forward(x, net.w, K, -1.0, act)[1], h_ref) > 100 * TOL


def test_state_crosses_replayed_graphs(dev):
    """T + K - 1 = 141 diagonals = 71 graph frames: one 64-frame graph and seven single ones, then a second call."""
    B, F, H, K = 2, 5, 8, 2
    cuts = (140, 7)
    rng = np.random.default_rng(9)
    net = Net(dev, F, H, K, seed=5)
    x = rng.random((B, sum(cuts), F)).astype(np.float32)
    x[1, 100:] = -1.0
    h, states = net.chunks(x, cuts, net.state(B))
    whole = net.run(x)
    torch.cuda.synchronize()
    _, h_ref = R.model_forward(x, net.w, K)
    _check(h.cpu().numpy(), h_ref, "hidden, chunked")
    assert torch.equal(h, whole)
    for (fh, fc), (rh, rc) in zip(states, _ref_states(net, x, cuts)):
        _check(fh, rh, "final_h")
        _check(fc, rc, "final_c")


def test_same_buffers_new_state_contents(dev):
    """The replayed graphs hold no state: the same shapes, workspace, output and state BUFFERS called twice with
    different state contents -- the second result follows the second state."""
    from drnmf_amd import ops
    B, T, F, H, K = 3, 5, 9, 10, 2
    rng = np.random.default_rng(13)
    net = Net(dev, F, H, K, seed=2)
    x, _ = R.masked_input(rng, B, T, F)
    xd = torch.from_numpy(x).to(dev)
    desc = ops.make_lstm_desc(B, T, F, H, K)
    ws = ops.lstm_workspace(desc, dev)
    out = torch.empty((B, T, ops.lstm_hidden_ld(H)), dtype=torch.float32, device=dev)[..., :H]
    ini, fin = net.state(B), net.state(B)
    for trial in range(2):
        st0 = SR.random_state(rng, K, B, H)
        for t, v in zip(ini, st0):
            t.copy_(torch.from_numpy(v))
        ops.lstm_forward(xd, -1.0, net.params, desc, out=out, workspace=ws, initial_state=ini, final_state=fin)
        torch.cuda.synchronize()
        _, h_ref, (rh, rc) = SR.model_forward(x, net.w, K, state=st0)
        _check(out.cpu().numpy(), h_ref, "hidden, trial %d" % trial)
        _check(fin[0].cpu().numpy(), rh, "final_h, trial %d" % trial)
        _check(fin[1].cpu().numpy(), rc, "final_c, trial %d" % trial)
        assert np.array_equal(ini[0].cpu().numpy(), st0[0]) and np.array_equal(ini[1].cpu().numpy(), st0[1])


def test_masking_across_chunks(dev):
    """Row A: valid frames end inside chunk 1, fully masked in chunk 2.  Row B: fully masked in chunk 1, valid in
    chunk 2.  Row C: never masked.  A row masked for a whole call leaves with exactly the state it entered with;
    h_out at masked frames before the first valid one is the carried h."""
    B, F, H, K = 3, 9, 10, 2
    cuts = (6, 5)
    rng = np.random.default_rng(17)
    net = Net(dev, F, H, K, seed=8)
    x = (1.0 - rng.random((B, sum(cuts), F))).astype(np.float32)
    x[0, 4:] = -1.0
    x[1, :6] = -1.0
    x[1, 6:8] = -1.0             # ... and two leading masked frames in chunk 2
    st0 = SR.random_state(rng, K, B, H)
    st = net.state(B, st0)
    h, states = net.chunks(x, cuts, st)
    torch.cuda.synchronize()
    h = h.cpu().numpy()
    (h1, c1), (h2, c2) = states
    assert np.array_equal(h1[:, 1], st0[0][:, 1]) and np.array_equal(c1[:, 1], st0[1][:, 1])     # B over chunk 1
    assert np.array_equal(h2[:, 0], h1[:, 0]) and np.array_equal(c2[:, 0], c1[:, 0])             # A over chunk 2
    for t in range(8):                       # B: the carried h until its first valid frame (frame 8)
        assert np.array_equal(h[1, t], st0[0][-1, 1]), t
    for t in range(6, 11):                   # A in chunk 2: the output chunk 1 ended on
        assert np.array_equal(h[0, t], h1[-1, 0]), t
    assert np.array_equal(h[0, 5], h[0, 3])
    _, h_ref, (rh, rc) = SR.chunked_forward(x, cuts, net.w, K, state=st0)
    _check(h, h_ref, "hidden")
    _check(h2, rh, "final_h")
    _check(c2, rc, "final_c")
    one = net.run(x, initial_state=net.state(B, st0))
    assert np.array_equal(one.cpu().numpy(), h)


def test_final_may_alias_initial(dev):
    B, F, H, K = 17, 33, 24, 3
    rng = np.random.default_rng(19)
    net = Net(dev, F, H, K, seed=4)
    x, _ = R.masked_input(rng, B, 5, F)
    st0 = SR.random_state(rng, K, B, H)
    ini, fin, both = net.state(B, st0), net.state(B), net.state(B, st0)
    for train in (False, True):
        for t, v in zip(both, st0):
            t.copy_(torch.from_numpy(v))
        a = net.run(x, train=train, initial_state=ini, final_state=fin)
        b = net.run(x, train=train, initial_state=both, final_state=both)
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        assert torch.equal(fin[0], both[0]) and torch.equal(fin[1], both[1])
        assert np.array_equal(ini[0].cpu().numpy(), st0[0])


def test_null_state_pointers(dev):
    """initial = NULL is the zero state, bit for bit, and the stateless entry point's result; final = NULL writes
    nothing: a call that is given only the entering buffers leaves them as they were, and h or c alone can be
    asked for."""
    B, F, H, K = 3, 9, 10, 2
    rng = np.random.default_rng(23)
    net = Net(dev, F, H, K, seed=6)
    x, _ = R.masked_input(rng, B, 5, F)
    for train in (False, True):
        plain = net.run(x, train=train)
        fin = net.state(B)
        a = net.run(x, train=train, final_state=fin)                         # initial NULL
        fz = net.state(B)
        b = net.run(x, train=train, initial_state=net.state(B), final_state=fz)
        torch.cuda.synchronize()
        assert torch.equal(a, plain) and torch.equal(b, plain)
        assert torch.equal(fin[0], fz[0]) and torch.equal(fin[1], fz[1])
        assert torch.equal(fin[0][-1], plain[:, -1])
        st0 = SR.random_state(rng, K, B, H)
        ini = net.state(B, st0)
        c = net.run(x, train=train, initial_state=ini)                       # final NULL
        guard = tuple(torch.full((K, B, H), 7.5, dtype=torch.float32, device=dev) for _ in range(2))
        d = net.run(x, train=train, initial_state=ini, final_state=(guard[0], None))
        e = net.run(x, train=train, initial_state=(ini[0], None), final_state=(None, guard[1]))
        torch.cuda.synchronize()
        assert np.array_equal(ini[0].cpu().numpy(), st0[0]) and np.array_equal(ini[1].cpu().numpy(), st0[1])
        assert torch.equal(c, d) and torch.equal(guard[0][-1], d[:, -1])
        _, _, (_, rc) = SR.model_forward(x, net.w, K, state=(st0[0], np.zeros_like(st0[1])))
        _check(guard[1].cpu().numpy(), rc, "final_c with initial_c = NULL")
        assert not torch.equal(e, c)


# ---- training -------------------------------------------------------------------------------------------------

def _model(dev, F, H, K, act="hard_sigmoid", seed=0, scale=1.5, stateful=True, compile_=True, **opt):
    from drnmf_amd import layers
    m = layers.build_lstm(dict(mask_value=-1.0, maxseq=8, input_dim=F, output_dim=F, K_layers=K, hidden_dim=H,
                               recurrent_activation=act, stateful=stateful), device=dev)
    w = R.random_weights(np.random.default_rng(seed), F, H, K, scale=scale)
    m.set_weights(w)
    if compile_:
        m.compile(**opt)
    return m, w


def _set_state(m, B, st0):
    for t, v in zip(m._state(B), st0):
        t.copy_(torch.from_numpy(v))


TRAIN_CASES = {"plain": dict(scale=1.5), "masked_t0": dict(scale=1.5, mask_t0=True), "saturated": dict(scale=8.0)}


@pytest.mark.parametrize("case", sorted(TRAIN_CASES))
def test_gradients_with_an_entering_state_match_autograd(dev, case):
    """B = 3, T = 6, F = 9, H = 10, K = 2 with an entering state of magnitude about 1 (a constant of the gradient);
    masked_t0: row 1 is masked at t = 0 (and row 2 for the whole call); saturated: hard-sigmoid gates pushed
    outside +-2.5 by 8x weights."""
    B, T, F, H, K = 3, 6, 9, 10, 2
    cfg = TRAIN_CASES[case]
    rng = np.random.default_rng(31)
    x = (1.0 - rng.random((B, T, F))).astype(np.float32)
    y = rng.random((B, T, F)).astype(np.float32)
    sw = np.ones((B, T), np.float32)
    if cfg.get("mask_t0"):
        x[1, :2] = -1.0
        x[2] = -1.0
        sw[1, :2] = 0.0
        sw[2, 3:] = 0.0           # (masked frames that still carry weight: xm = 0 there, the loss is w mean y^2)
    m, w = _model(dev, F, H, K, seed=12, scale=cfg["scale"])
    if case == "saturated":
        z0 = torch.as_tensor(x, dtype=torch.float64) @ torch.as_tensor(w[0], dtype=torch.float64)
        assert float((z0.abs() > 2.5).double().mean()) > 0.3
    st0 = SR.random_state(rng, K, B, H)
    _set_state(m, B, st0)
    t = lambda a: torch.from_numpy(a).to(dev)
    flat = m.loss_and_grads(t(x), t(y), t(sw))
    torch.cuda.synchronize()
    f = flat.cpu().numpy()
    gs = [m._gview[n].cpu().numpy() for n, _ in m._train_items]
    sse_r, cnt_r, gr, (rh, rc) = SR.loss_and_grads(x, y, sw, w, K, state=st0)
    assert float(f[-3]) == cnt_r
    print("%s: loss rel err %.3e" % (case, abs(float(f[-4]) - sse_r) / abs(sse_r)))
    for g, r, (n, _) in zip(gs, gr, m._train_items):
        print("%s: %s max|d|/max|ref| = %.3e" % (case, n, _rel(g, r)))
    assert abs(float(f[-4]) - sse_r) <= L_TOL * abs(sse_r)
    for g, r, (n, _) in zip(gs, gr, m._train_items):
        assert _rel(g, r) <= G_TOL, "%s: max|d|/max|ref| = %.3e" % (n, _rel(g, r))
    _check(m._states[0].cpu().numpy(), rh, "final_h")
    _check(m._states[1].cpu().numpy(), rc, "final_c")


def test_training_forward_with_state_is_bit_identical(dev):
    B, T, F, H, K = 17, 7, 33, 24, 3
    rng = np.random.default_rng(37)
    net = Net(dev, F, H, K, seed=9)
    x, _ = R.masked_input(rng, B, T, F)
    st0 = SR.random_state(rng, K, B, H)
    fa, fb = net.state(B), net.state(B)
    a = net.run(x, initial_state=net.state(B, st0), final_state=fa)
    b = net.run(x, train=True, initial_state=net.state(B, st0), final_state=fb)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(fa[0], fb[0]) and torch.equal(fa[1], fb[1])


# ---- model level ------------------------------------------------------------------------------------------------

def test_model_chunked_predict_reset_and_batch_size(dev):
    B, F, H, K = 5, 20, 13, 2
    cuts = (4, 7, 5)
    rng = np.random.default_rng(43)
    x, _ = R.masked_input(rng, B, sum(cuts), F)
    ms, w = _model(dev, F, H, K, seed=1, compile_=False)
    mp, _ = _model(dev, F, H, K, seed=1, stateful=False, compile_=False)
    one = ms.predict_on_batch(x)
    plain = mp.predict_on_batch(x)
    assert np.array_equal(one, plain)                   # from zero states: the stateless model, bit for bit
    y_ref, _ = R.model_forward(x, w, K)
    _check(one, y_ref, "one-shot")
    assert not np.array_equal(ms.predict_on_batch(x), one)          # the state has moved on
    ms.reset_states()
    assert np.array_equal(ms.predict_on_batch(x), one)              # reset: the zero-state result again
    ms.reset_states()
    t0, parts = 0, []
    for n in cuts:
        parts.append(ms.predict_on_batch(x[:, t0:t0 + n]))
        t0 += n
    chunked = np.concatenate(parts, axis=1)
    np.testing.assert_allclose(chunked, one, rtol=0, atol=1e-6)
    _check(chunked, y_ref, "chunked")
    with pytest.raises(ValueError):
        ms.predict_on_batch(x[:3])
    ms.reset_states(batch_size=3)
    assert np.array_equal(ms.predict_on_batch(x[:3]), plain[:3])
    # predict keeps row order and carries row i to row i of the next batch
    ms.reset_states(batch_size=B)
    two = ms.predict(np.concatenate([x[:, :8], x[:, 8:]], axis=0), batch_size=B)
    np.testing.assert_allclose(np.concatenate([two[:B], two[B:]], axis=1), one, rtol=0, atol=1e-6)
    with pytest.raises(NotImplementedError):
        ms.enhance([np.zeros(2048, np.int16)], N=2 * (F - 1), hop=F - 1)


def test_train_on_batch_carries_the_state(dev):
    """Two steps on consecutive cuts: the second step's loss is the reference's with the weights after the first
    step and the state the first step's forward left -- not the zero-state one."""
    B, T, F, H, K = 4, 6, 9, 10, 2
    rng = np.random.default_rng(47)
    x = (1.0 - rng.random((B, 2 * T, F))).astype(np.float32)
    y = rng.random((B, 2 * T, F)).astype(np.float32)
    sw = np.ones((B, T), np.float32)
    m, w = _model(dev, F, H, K, seed=14, lr=1e-3)
    l1 = float(m.train_on_batch(x[:, :T], y[:, :T], sw))
    sse1, cnt1, _, st1 = SR.loss_and_grads(x[:, :T], y[:, :T], sw, w, K)
    assert abs(l1 - sse1 / cnt1) <= L_TOL * sse1 / cnt1
    _check(m._states[0].cpu().numpy(), st1[0], "state after step 1, h")
    _check(m._states[1].cpu().numpy(), st1[1], "state after step 1, c")
    w1 = m.get_weights()
    carried = tuple(s.cpu().numpy() for s in m._states)
    l2 = float(m.train_on_batch(x[:, T:], y[:, T:], sw))
    sse2, cnt2, _, _ = SR.loss_and_grads(x[:, T:], y[:, T:], sw, w1, K, state=carried)
    sse0, _, _, _ = SR.loss_and_grads(x[:, T:], y[:, T:], sw, w1, K)
    assert abs(l2 - sse2 / cnt2) <= L_TOL * sse2 / cnt2
    assert abs(sse0 - sse2) > 10 * L_TOL * sse2           # the zero-state loss lies outside the bound above, tenfold
    # test_on_batch carries too
    m.reset_states()
    a = m.test_on_batch(x[:, :T], y[:, :T], sw)
    b = m.test_on_batch(x[:, :T], y[:, :T], sw)
    assert a != b
    with pytest.raises(ValueError):
        m.train_on_batch(x[:2, :T], y[:2, :T], sw[:2])


def test_fit_validation_leaves_the_training_state(dev):
    """The rule: validation inside fit() runs on a state of its own, from zero (here at another batch size, which
    the training state would refuse); fit() leaves the state behind its last training batch -- that of the same
    fit without validation data, bit for bit."""
    B, T, F, H, K = 4, 6, 9, 10, 2
    rng = np.random.default_rng(53)
    x = (1.0 - rng.random((2 * B, T, F))).astype(np.float32)
    y = rng.random((2 * B, T, F)).astype(np.float32)
    sw = np.ones((2 * B, T), np.float32)
    xv, yv, wv = x[:3] * 0.5, y[:3], sw[:3]
    kw = dict(sample_weight=sw, batch_size=B, epochs=2, shuffle=False)
    m1, _ = _model(dev, F, H, K, seed=15, lr=1e-3)
    m2, _ = _model(dev, F, H, K, seed=15, lr=1e-3)
    h1 = m1.fit(x, y, validation_data=(xv, yv, wv), **kw)
    h2 = m2.fit(x, y, **kw)
    torch.cuda.synchronize()
    assert len(h1["val_loss"]) == 2 and h1["loss"] == h2["loss"]
    assert tuple(m1._states[0].shape) == (K, B, H)
    assert torch.equal(m1._states[0], m2._states[0]) and torch.equal(m1._states[1], m2._states[1])
    assert float(m1._states[0].abs().max()) > 0
