"""The LSTM baseline (csrc/lstm.hip) on the GPU at the lengths, masks and shapes it meets, against the fp64
reference (tests/lstm_ref.py), in both matrix modes of the frame-parallel products (the input projection and the
head follow the handle's mode; the recurrence is exact-fp32 MFMA either way).

  - lengths that cross the frame-graph chunking of drnmf_lstm_forward: T + K - 1 diagonals, paired into frames,
    replayed as graphs of min(frames, 64) frames plus single-frame graphs for the remainder, with the diagonal
    counters carried from one replay to the next -- up to the measured configuration (T = 500) and T = 2000;
  - masked frames anywhere in a sequence (leading, interior, trailing, all), partly masked frames, mask_value 0;
  - shape edges of the tiling (T = 1, K > T, F <= 5, H across the 8-unit tiles and 16-row contraction chunks,
    B across the 16-row tiles), the output contract (caller strides, held outputs, the graph cache), and
    saturated / kinked / large / non-finite inputs.

Tolerance: max|d| / max|ref| <= 1e-4, as in tests/test_gpu_lstm.py.
"""
import numpy as np
import pytest
import torch

import lstm_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4
ACTS = ["hard_sigmoid", "sigmoid"]


def _rup(v, m):
    return (v + m - 1) // m * m


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (run with -m 'not gpu' on CPU boxes)")
    from drnmf_amd import _capi
    _capi.handle(0)
    return torch.device("cuda:0")


@pytest.fixture(params=["f32", "bf16x3"])
def mode(request, dev):
    """The handle's matrix mode for the test, the previous one restored afterwards."""
    from drnmf_amd import ops
    prev = ops.set_matrix_mode(request.param, dev)
    yield request.param
    ops.set_matrix_mode(prev, dev)


def _check(got, ref, what):
    scale = max(float(np.max(np.abs(ref))), 1e-30)
    err = float(np.max(np.abs(got - ref))) / scale
    assert err <= TOL, "%s: max|d|/max|ref| = %.3e" % (what, err)


def _model(dev, w, K, act="hard_sigmoid", mask_value=-1.0):
    from drnmf_amd import layers
    F, H = w[0].shape[0], w[1].shape[0]
    m = layers.build_lstm(dict(mask_value=mask_value, maxseq=8, input_dim=F, output_dim=F, K_layers=K,
                               hidden_dim=H, recurrent_activation=act), device=dev)
    m.set_weights(w)
    return m


def _fwd(m, x, dev):
    """model.forward -> (output, hidden) as numpy"""
    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(dev)
    y, h = m.forward(xd, want_hidden=True)
    torch.cuda.synchronize()
    return y.cpu().numpy(), h.cpu().numpy()


def _run_and_check(dev, x, w, K, act, mask_value=-1.0, rows=None, what=""):
    m = _model(dev, w, K, act, mask_value)
    y, h = _fwd(m, x, dev)
    y_ref, h_ref = R.model_forward(x, w, K, mask_value, act, rows=rows)
    if rows is not None:
        y, h = y[rows], h[rows]
    _check(h, h_ref, what + " hidden")
    _check(y, y_ref, what + " output")
    return m, y, h


# ---- lengths across the graph chunks -------------------------------------------------------------------------

# (T, K) -> frames = (T + K) // 2: 63 (one graph), exactly 64, 64 + 1 remainder, 64 + 37 remainders
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("T,K", [(126, 1), (128, 1), (129, 1), (200, 3)], ids=lambda v: str(v))
def test_graph_chunks_and_remainder_frames(dev, mode, T, K, act):
    B, F, H = 7, 33, 24
    rng = np.random.default_rng(T * 10 + K)
    x, _ = R.masked_input(rng, B, T, F)
    w = R.random_weights(rng, F, H, K, scale=1.5)
    m, y, h = _run_and_check(dev, x, w, K, act)
    y2, h2 = _fwd(m, x, dev)               # the cached graphs again: the counters restart at diagonal 0
    assert np.array_equal(h, h2) and np.array_equal(y, y2)


# rows checked in the measured configuration: both sides of the first 16-row tile boundary, the last tile, an
# all-masked row and rows with interior, leading and partly masked frames
BENCH_ROWS = [0, 15, 16, 17, 248, 249, 100, 101]


@pytest.mark.parametrize("act", ACTS)
def test_measured_configuration(dev, mode, act):
    """B = 250, T = 500, F = 513, H = 250, K = 5 (profiles/lstm_bench.jsonl): 504 diagonals = the 64-frame graph
    three times, then 60 single-frame replays.  Rows other than BENCH_ROWS hold the reference's layout (valid
    prefix, -1 padding); BENCH_ROWS take the patterns of masked_input ('mixed': none, trailing, leading,
    interior, partial, all, combo, none)."""
    B, T, F, H, K = 250, 500, 513, 250, 5
    rng = np.random.default_rng(500)
    g = torch.Generator(device=dev)
    g.manual_seed(500)
    x = torch.rand((B, T, F), device=dev, generator=g)
    lens = torch.from_numpy(rng.integers(1, T + 1, size=B)).to(dev)
    x[torch.arange(T, device=dev)[None, :] >= lens[:, None]] = -1.0
    xs, valid = R.masked_input(rng, len(BENCH_ROWS), T, F)
    assert not valid[5].any() and not valid[3, 1:-1].all()
    x[BENCH_ROWS] = torch.from_numpy(xs).to(dev)
    w = R.random_weights(rng, F, H, K, scale=1.5)
    m = _model(dev, w, K, act)
    y, h = m.forward(x, want_hidden=True)
    idx = torch.tensor(BENCH_ROWS, device=dev)
    y, h = y[idx].cpu().numpy(), h[idx].cpu().numpy()
    y_ref, h_ref = R.model_forward(xs, w, K, -1.0, act)
    _check(h, h_ref, "hidden")
    _check(y, y_ref, "output")
    assert float(np.abs(h[5]).max()) == 0.0


def test_reference_length_does_not_drift(dev, mode):
    """T = 2000 frames, every row checked: the error per frame over the last 100 frames stays at the level of the
    first 100 (the state carries fp32 rounding along 2000 dependent steps per layer)."""
    B, T, F, H, K = 4, 2000, 513, 54, 2
    rng = np.random.default_rng(2000)
    x, _ = R.masked_input(rng, B, T, F)
    w = R.random_weights(rng, F, H, K, scale=1.5)
    m = _model(dev, w, K)
    y, h = _fwd(m, x, dev)
    y_ref, h_ref = R.model_forward(x, w, K)
    _check(y, y_ref, "output")
    err_t = np.max(np.abs(h - h_ref), axis=(0, 2)) / np.max(np.abs(h_ref))
    assert err_t.max() <= TOL, "hidden: %.3e" % err_t.max()
    assert err_t[-100:].max() <= 4 * max(err_t[:100].max(), 1e-7), \
        "error grows with t: first 100 frames %.3e, last 100 %.3e" % (err_t[:100].max(), err_t[-100:].max())


def test_graph_replay_equals_direct_launches_at_length(dev, mode, monkeypatch):
    """T = 300, K = 3: 151 frames = two 64-frame replays and 23 single-frame ones, bit-identical to the same
    launches made directly (DRNMF_NO_GRAPH=1)."""
    B, T, F, H, K = 20, 300, 65, 40, 3
    rng = np.random.default_rng(300)
    x, _ = R.masked_input(rng, B, T, F)
    w = R.random_weights(rng, F, H, K, scale=1.5)
    m = _model(dev, w, K, "sigmoid")
    xd = torch.from_numpy(x).to(dev)
    a = _fwd(m, xd, dev)
    b = _fwd(m, xd, dev)
    monkeypatch.setenv("DRNMF_NO_GRAPH", "1")
    c = _fwd(m, xd, dev)
    for u, v in ((a, b), (a, c)):
        assert np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1])
    rows = [0, 3, 6, 13, 19]
    y_ref, h_ref = R.model_forward(x, w, K, -1.0, "sigmoid", rows=rows)
    _check(a[1][rows], h_ref, "hidden")
    _check(a[0][rows], y_ref, "output")


# ---- masking semantics ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("mask_value", [-1.0, 0.0])
def test_masking_patterns(dev, mode, mask_value, K, act):
    """Leading, interior and trailing masked runs, all-masked rows and partly masked frames (every bin but one
    = mask_value: valid), in 21 rows over two 16-row tiles.  A masked frame's hidden row is the previous frame's
    exactly, zero before the first valid frame; predict (length-aware) equals the plain padded run."""
    B, T, F, H = 21, 37, 45, 20
    rng = np.random.default_rng(K * 10 + int(mask_value == 0))
    x, valid = R.masked_input(rng, B, T, F, "mixed", mask_value)
    w = R.random_weights(rng, F, H, K, scale=1.5)
    m, y, h = _run_and_check(dev, x, w, K, act, mask_value)
    for b in range(B):
        for t in np.nonzero(~valid[b])[0]:
            if valid[b, :t].any():
                assert np.array_equal(h[b, t], h[b, t - 1]), (b, t)
            else:
                assert float(np.abs(h[b, t]).max()) == 0.0, (b, t)
    out = m.predict(x, batch_size=8)
    padded = m.predict(x, batch_size=8, length_aware=False)
    np.testing.assert_allclose(out, padded, rtol=0, atol=1e-6)
    _check(out, R.model_forward(x, w, K, mask_value, act)[0], "predict")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("K", [1, 3])
def test_mask_value_none_takes_every_frame(dev, mode, K, act):
    """ops.lstm_forward with mask_value None: frames of -1 (or of 0) everywhere are ordinary input."""
    from drnmf_amd import ops
    B, T, F, H = 9, 23, 30, 20
    rng = np.random.default_rng(40 + K)
    x, _ = R.masked_input(rng, B, T, F, "mixed", -1.0)
    x[1, 3:6] = 0.0
    w = R.random_weights(rng, F, H, K, scale=1.5)
    desc = ops.make_lstm_desc(B, T, F, H, K, act)
    t = lambda a: torch.from_numpy(a).to(dev)
    p = ops.lstm_prepare_params(desc, [t(a) for a in w[0:3 * K:3]], [t(a) for a in w[1:3 * K:3]],
                                [t(a) for a in w[2:3 * K:3]], t(w[-2]), t(w[-1]))
    h = ops.lstm_forward(t(x), None, p, desc)
    y = ops.lstm_head_forward(h, p, desc)
    torch.cuda.synchronize()
    y_ref, h_ref = R.model_forward(x, w, K, None, act)
    _check(h.cpu().numpy(), h_ref, "hidden")
    _check(y.cpu().numpy(), y_ref, "output")


# ---- shape edges ---------------------------------------------------------------------------------------------

# (B, T, F, H, K, rows checked or None for all)
SHAPES = [(5, 1, 33, 20, 2, None), (16, 1, 513, 54, 5, None), (6, 2, 33, 20, 5, None)] + \
    [(5, 9, F, 20, 2, None) for F in (1, 3, 4, 5)] + \
    [(5, 7, 20, H, 2, None) for H in (1, 8, 16, 17, 64, 256, 257, 512)] + \
    [(20, 7, 20, 1000, 2, [0, 3, 15, 16, 19])] + \
    [(B, 6, 33, 20, 2, None) for B in (15, 16, 17, 255, 256, 257)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%dT%dF%dH%dK%d" % s[:5])
def test_shape_edges(dev, mode, shape):
    B, T, F, H, K, rows = shape
    act = ACTS[(B + T + F + H + K) % 2]
    rng = np.random.default_rng(B * 7 + T * 5 + F * 3 + H + K)
    x, _ = R.masked_input(rng, B, T, F)
    w = R.random_weights(rng, F, H, K, scale=1.5)
    _run_and_check(dev, x, w, K, act, rows=rows)


# ---- output contract -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", [13, 250])
def test_caller_out_with_its_own_row_stride(dev, mode, H):
    """A caller's out with ld_h in {H, H + 1, round_up(H, 4), round_up(H, 4) + 4, round_up(H, 8) + 8}, prefilled
    with NaN: columns [0, H) are the hidden states, [H, min(ld_h, round_up(H, 4))) are written 0 (the head
    contracts them when ld_h >= round_up(H, 4)), and the head on that buffer is finite and right."""
    from drnmf_amd import ops
    B, T, F, K = 5, 11, 40, 2
    rng = np.random.default_rng(H)
    x, _ = R.masked_input(rng, B, T, F)
    w = R.random_weights(rng, F, H, K, scale=1.5)
    y_ref, h_ref = R.model_forward(x, w, K)
    desc = ops.make_lstm_desc(B, T, F, H, K)
    t = lambda a: torch.from_numpy(a).to(dev)
    p = ops.lstm_prepare_params(desc, [t(a) for a in w[0:3 * K:3]], [t(a) for a in w[1:3 * K:3]],
                                [t(a) for a in w[2:3 * K:3]], t(w[-2]), t(w[-1]))
    xd = t(x)
    Hq = _rup(H, 4)
    for ld in sorted({H, H + 1, Hq, Hq + 4, _rup(H, 8) + 8}):
        buf = torch.full((B, T, ld), float("nan"), device=dev)
        out = buf[..., :H]
        r = ops.lstm_forward(xd, -1.0, p, desc, out=out)
        assert r.data_ptr() == buf.data_ptr()
        y = ops.lstm_head_forward(out, p, desc)
        torch.cuda.synchronize()
        b = buf.cpu().numpy()
        _check(b[..., :H], h_ref, "hidden, ld_h %d" % ld)
        assert np.all(b[..., H:min(ld, Hq)] == 0.0), "ld_h %d: padding columns not zero" % ld
        yn = y.cpu().numpy()
        assert np.isfinite(yn).all(), "ld_h %d: head not finite" % ld
        _check(yn, y_ref, "head, ld_h %d" % ld)


def test_held_output_survives_a_second_forward(dev, mode):
    """Outputs of one forward, still held, are not touched by the next forward of the same shape (whose hidden
    buffer is then a different allocation: the cached graph must write there, not into the held one)."""
    B, T, F, H, K = 6, 50, 40, 24, 2
    rng = np.random.default_rng(77)
    x1, _ = R.masked_input(rng, B, T, F)
    x2, _ = R.masked_input(rng, B, T, F)
    w = R.random_weights(rng, F, H, K, scale=1.5)
    m = _model(dev, w, K)
    y1, h1 = m.forward(torch.from_numpy(x1).to(dev), want_hidden=True)
    y1c, h1c = y1.clone(), h1.clone()
    y2, h2 = m.forward(torch.from_numpy(x2).to(dev), want_hidden=True)
    torch.cuda.synchronize()
    assert torch.equal(y1, y1c) and torch.equal(h1, h1c)
    y_ref, h_ref = R.model_forward(x2, w, K)
    _check(h2.cpu().numpy(), h_ref, "second hidden")
    _check(y2.cpu().numpy(), y_ref, "second output")
    _check(y1.cpu().numpy(), R.model_forward(x1, w, K)[0], "first output")


def test_alternating_shapes_on_one_model(dev, mode):
    """(B, T) = (32, 300) and (3, 40) in turn on one model (one workspace, two cached graph sets): every result
    equals that shape's first result bit for bit."""
    F, H, K = 65, 40, 3
    rng = np.random.default_rng(32)
    w = R.random_weights(rng, F, H, K, scale=1.5)
    m = _model(dev, w, K)
    xa, _ = R.masked_input(rng, 32, 300, F)
    xb, _ = R.masked_input(rng, 3, 40, F)
    xad, xbd = torch.from_numpy(xa).to(dev), torch.from_numpy(xb).to(dev)
    ra, rb = _fwd(m, xad, dev), _fwd(m, xbd, dev)
    rows = [0, 5, 16, 31]
    y_ref, h_ref = R.model_forward(xa, w, K, rows=rows)
    _check(ra[1][rows], h_ref, "hidden (32, 300)")
    _check(ra[0][rows], y_ref, "output (32, 300)")
    y_ref, h_ref = R.model_forward(xb, w, K)
    _check(rb[1], h_ref, "hidden (3, 40)")
    _check(rb[0], y_ref, "output (3, 40)")
    for _ in range(2):
        for xd, r in ((xad, ra), (xbd, rb)):
            y, h = _fwd(m, xd, dev)
            assert np.array_equal(y, r[0]) and np.array_equal(h, r[1])


# ---- numeric edges -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("act", ACTS)
def test_saturated_gates(dev, mode, act):
    """kernel_0 at scale 20 and a quarter of every layer's gate biases at +-100: pre-activations reach +-100,
    where expf(-z) overflows inside the sigmoid and tanh saturates.  (The recurrent kernels stay at scale 1.5:
    at scale 20 the recurrence itself is chaotic and fp32 cannot follow fp64 however it is computed.)"""
    B, T, F, H, K = 6, 40, 513, 64, 2
    rng = np.random.default_rng(20)
    w = R.random_weights(rng, F, H, K, scale=1.5)
    w[0] = R.random_weights(rng, F, H, 1, scale=20.0)[0]
    for k in range(K):
        sel = rng.random(4 * H) < 0.25
        w[3 * k + 2][sel] = rng.choice([-100.0, 100.0], size=int(sel.sum()))
    x, _ = R.masked_input(rng, B, T, F)
    m, y, h = _run_and_check(dev, x, w, K, act)
    assert np.isfinite(y).all() and np.isfinite(h).all()


def test_hard_sigmoid_kinks(dev, mode):
    """Gate biases at exactly +-2.5 with small weights: the pre-activations sit on and around the kinks of
    hard_sigmoid (exactly on them for all-zero frames at t = 0, where h = 0)."""
    B, T, F, H, K = 7, 30, 40, 24, 2
    rng = np.random.default_rng(25)
    w = R.random_weights(rng, F, H, K, scale=0.01)
    for k in range(K):
        w[3 * k + 2][:] = rng.choice([-2.5, 2.5], size=4 * H)
    x, _ = R.masked_input(rng, B, T, F)
    x[0, :3] = 0.0
    _run_and_check(dev, x, w, K, "hard_sigmoid")


@pytest.mark.parametrize("act", ACTS)
def test_large_inputs(dev, mode, act):
    """Bins log-uniform up to 1e4, like unnormalised STFT magnitudes (kernel_0 scaled by 1e-3 so that the
    pre-activations are O(1) -- a model trained on such input has small input weights)."""
    B, T, F, H, K = 6, 40, 513, 64, 2
    rng = np.random.default_rng(10000)
    w = R.random_weights(rng, F, H, K, scale=1.5)
    w[0] = w[0] * np.float32(1e-3)
    x, valid = R.masked_input(rng, B, T, F)
    mag = (10.0 ** rng.uniform(-1, 4, size=x.shape)).astype(np.float32)
    x[valid] = (x * mag)[valid]
    assert x.max() > 5e3
    _run_and_check(dev, x, w, K, act)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_bin_stays_in_its_row(dev, mode, bad):
    """One NaN / Inf bin in one frame of one row: that row may go non-finite from that frame on, every other
    row (the rest of its 16-row tile included) stays finite and matches the reference, and the row itself
    matches it before that frame."""
    B, T, F, H, K = 20, 30, 65, 40, 2
    rng = np.random.default_rng(99)
    x, valid = R.masked_input(rng, B, T, F)
    w = R.random_weights(rng, F, H, K, scale=1.5)
    r = 4
    t0 = int(np.nonzero(valid[r, T // 3:])[0][0]) + T // 3
    x[r, t0, 7] = bad
    m = _model(dev, w, K)
    y, h = _fwd(m, x, dev)
    y_ref, h_ref = R.model_forward(x, w, K)
    others = [b for b in range(B) if b != r]
    assert np.isfinite(h[others]).all() and np.isfinite(y[others]).all()
    _check(h[others], h_ref[others], "hidden, other rows")
    _check(y[others], y_ref[others], "output, other rows")
    _check(h[r, :t0], h_ref[r, :t0], "hidden, the row before the bad frame")
    _check(y[r, :t0], y_ref[r, :t0], "output, the row before the bad frame")
