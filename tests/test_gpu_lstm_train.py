"""Training of the LSTM baseline on the GPU (enhance.py:1260-1312; csrc/lstm.hip training forward, loss head,
BPTT as a reverse wavefront): gradients against fp64 autograd of tests/lstm_train_ref.py, the Adam step, fit
with the reference's callbacks, the prepared block after a step, determinism.

Tolerances: gradients max|d| / max|ref| <= G_TOL per weight array (as test_gpu_train.py), the loss 1e-5 relative;
where hard_sigmoid kinks can flip in fp32 (saturated gates) a norm-based bound instead.
"""
import os
import pickle

import numpy as np
import pytest
import torch

import lstm_ref as R
import lstm_train_ref as TR

pytestmark = pytest.mark.gpu

G_TOL = 2e-3
L_TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (run with -m 'not gpu' on CPU boxes)")
    from drnmf_amd import _capi
    _capi.handle(0)
    return torch.device("cuda:0")


def _model(dev, F, H, K, act="hard_sigmoid", seed=0, scale=1.0, mask_value=-1.0, **opt):
    from drnmf_amd import layers
    m = layers.build_lstm(dict(mask_value=mask_value, maxseq=8, input_dim=F, output_dim=F, K_layers=K,
                               hidden_dim=H, recurrent_activation=act), device=dev)
    w = R.random_weights(np.random.default_rng(seed), F, H, K, scale=scale)
    m.set_weights(w)
    m.compile(**opt)
    return m, w


def _data(rng, B, T, F, partial_weights=True):
    x, valid = R.masked_input(rng, B, T, F)
    y = rng.random((B, T, F)).astype(np.float32)
    w = valid.astype(np.float32)
    if partial_weights:                          # a few valid frames without weight, a few masked ones with
        w[rng.random((B, T)) < 0.1] = 0.0
        w[rng.random((B, T)) < 0.05] = 0.5
    return x, y, w


def _grads(m, dev, x, y, w):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    flat = m.loss_and_grads(t(x), t(y), t(w))
    torch.cuda.synchronize()
    f = flat.cpu().numpy()
    gs = [m._gview[n].cpu().numpy() for n, _ in m._train_items]
    return float(f[-4]), float(f[-3]), gs


def _check_grads(got, ref, names, tol=G_TOL):
    for g, r, n in zip(got, ref, names):
        scale = max(float(np.max(np.abs(r))), 1e-30)
        err = float(np.max(np.abs(g - r))) / scale
        assert err <= tol, "%s: max|d|/max|ref| = %.3e" % (n, err)


# (B, T, F, H, K): H not a multiple of 8 / 16, F not a multiple of 4, B not a multiple of 16
SMALL = [(3, 11, 18, 13, 1), (7, 9, 33, 20, 2), (17, 8, 21, 37, 3)]


@pytest.mark.parametrize("act", ["hard_sigmoid", "sigmoid"])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "B%dT%dF%dH%dK%d" % s)
def test_gradients_match_autograd(dev, shape, act):
    B, T, F, H, K = shape
    rng = np.random.default_rng(B + 10 * H)
    x, y, w = _data(rng, B, T, F)
    m, wt = _model(dev, F, H, K, act, seed=H, scale=1.5)
    sse, cnt, gs = _grads(m, dev, x, y, w)
    sse_r, cnt_r, gr = TR.loss_and_grads(x, y, w, wt, K, -1.0, act)
    assert cnt == cnt_r
    assert abs(sse - sse_r) <= L_TOL * abs(sse_r)
    _check_grads(gs, gr, [n for n, _ in m._train_items])


def test_gradients_big_shape_cross_graph_chunk(dev):
    """K = 5, H = 250, F = 513 and T = 140: 144 diagonals, more than one 64-frame graph of two diagonals."""
    B, T, F, H, K = 2, 140, 513, 250, 5
    rng = np.random.default_rng(5)
    x, y, w = _data(rng, B, T, F)
    m, wt = _model(dev, F, H, K, seed=3)
    sse, cnt, gs = _grads(m, dev, x, y, w)
    sse_r, cnt_r, gr = TR.loss_and_grads(x, y, w, wt, K)
    assert cnt == cnt_r
    assert abs(sse - sse_r) <= L_TOL * abs(sse_r)
    for g, r, n in zip(gs, gr, [n for n, _ in m._train_items]):
        rel = float(np.linalg.norm(g - r)) / max(float(np.linalg.norm(r)), 1e-30)
        assert rel <= G_TOL, "%s: |d|/|ref| = %.3e" % (n, rel)


def test_hard_sigmoid_saturation(dev):
    """Weights scaled so that many gate pre-activations lie outside +-2.5: those gates get no gradient."""
    B, T, F, H, K = 5, 12, 24, 19, 2
    rng = np.random.default_rng(11)
    x, y, w = _data(rng, B, T, F)
    m, wt = _model(dev, F, H, K, seed=4, scale=8.0)
    from drnmf_amd import ops
    xs = torch.as_tensor(x, dtype=torch.float64)
    z0 = (xs * R.valid_frames(xs, -1.0).unsqueeze(-1)) @ torch.as_tensor(wt[0], dtype=torch.float64)
    assert float((z0.abs() > 2.5).double().mean()) > 0.3           # the inputs really saturate
    sse, cnt, gs = _grads(m, dev, x, y, w)
    sse_r, cnt_r, gr = TR.loss_and_grads(x, y, w, wt, K)
    assert abs(sse - sse_r) <= L_TOL * abs(sse_r)
    for g, r, n in zip(gs, gr, [n for n, _ in m._train_items]):
        rel = float(np.linalg.norm(g - r)) / max(float(np.linalg.norm(r)), 1e-30)
        assert rel <= G_TOL, "%s: |d|/|ref| = %.3e" % (n, rel)


def test_training_forward_hidden_is_bit_identical(dev):
    from drnmf_amd import ops
    B, T, F, H, K = 19, 23, 40, 70, 3
    rng = np.random.default_rng(2)
    x, _ = R.masked_input(rng, B, T, F)
    m, _ = _model(dev, F, H, K, seed=1)
    xt = torch.from_numpy(x).to(dev)
    desc = m._desc(B, T)
    params = m._params(desc)
    h_inf = ops.lstm_forward(xt, -1.0, params, desc)
    h_tr = ops.lstm_train_forward(xt, -1.0, params, desc, ops.lstm_train_workspace(desc, dev))
    torch.cuda.synchronize()
    assert torch.equal(h_inf, h_tr)


def _adam_closed_form(p, g, lr, b1=0.9, b2=0.999, eps=1e-8):
    mt = (1 - b1) * g
    vt = (1 - b2) * g * g
    lr_t = lr * np.sqrt(1 - b2) / (1 - b1)
    return p - lr_t * mt / (np.sqrt(vt) + eps)


@pytest.mark.parametrize("clip", [0.0, "engaged"])
def test_train_on_batch_first_step_and_descent(dev, clip):
    B, T, F, H, K = 6, 10, 20, 16, 2
    rng = np.random.default_rng(3)
    x, y, w = _data(rng, B, T, F)
    m, wt = _model(dev, F, H, K, seed=6, lr=1e-4)
    sse_r, cnt_r, gr = TR.loss_and_grads(x, y, w, wt, K)
    g = [v / cnt_r for v in gr]
    norm = np.sqrt(sum(float(np.sum(v * v)) for v in g))
    if clip == "engaged":
        m.opt["clipnorm"] = 0.5 * norm
        g = [v * 0.5 for v in g]
    loss = float(m.train_on_batch(x, y, w))
    assert abs(loss - sse_r / cnt_r) <= L_TOL * abs(sse_r / cnt_r)
    after = m.get_weights()
    for p0, gg, p1 in zip(wt, g, after):
        want = _adam_closed_form(p0.astype(np.float64), gg, 1e-4)
        assert np.max(np.abs(p1 - p0)) <= 1e-4 * 1.001                 # Adam's first step is at most lr
        big = np.abs(gg) > 1e-3 * np.max(np.abs(gg))                    # (no sign flips of fp32 vs fp64 there)
        assert np.max(np.abs(p1 - want)[big]) <= 1e-6
    first = float(m.test_on_batch(x, y, w))
    for _ in range(14):
        m.train_on_batch(x, y, w)
    last = float(m.test_on_batch(x, y, w))
    assert last < first
    # test_on_batch agrees with the reference loss at the current weights
    sse2, cnt2, _ = TR.loss_and_grads(x, y, w, m.get_weights(), K)
    assert abs(last - sse2 / cnt2) <= 1e-5 * abs(sse2 / cnt2)


def test_predict_after_step_uses_new_weights(dev):
    """The fused Adam writes the weights through raw pointers: the prepared block must not be served stale."""
    B, T, F, H, K = 4, 9, 16, 12, 2
    rng = np.random.default_rng(8)
    x, y, w = _data(rng, B, T, F)
    m, _ = _model(dev, F, H, K, seed=9, lr=1e-2)
    xt = torch.from_numpy(x).to(dev)
    m.forward(xt)                                          # prepare the block for this shape
    m.train_on_batch(x, y, w)
    y_dev = m.forward(xt).cpu().numpy()
    y_ref, _ = R.model_forward(x, m.get_weights(), K)
    assert np.max(np.abs(y_dev - y_ref)) <= 1e-4 * np.max(np.abs(y_ref))
    y_pred = m.predict(x, batch_size=2)
    assert np.max(np.abs(y_pred - y_ref)) <= 1e-4 * np.max(np.abs(y_ref))


def test_unweighted_loss_uses_masking_output(dev):
    """sample_weight=None on ragged input: masked frames count, with the Masking layer's zeros (not raw x)."""
    B, T, F, H, K = 5, 12, 10, 9, 1
    rng = np.random.default_rng(12)
    x, _, _ = _data(rng, B, T, F)
    y = rng.random((B, T, F)).astype(np.float32)
    m, wt = _model(dev, F, H, K, seed=2, lr=1e-4)
    ones = np.ones((B, T), np.float32)
    sse_r, cnt_r, _ = TR.loss_and_grads(x, y, ones, wt, K)
    assert abs(float(m.test_on_batch(x, y)) - sse_r / cnt_r) <= L_TOL * sse_r / cnt_r
    assert abs(float(m.train_on_batch(x, y)) - sse_r / cnt_r) <= L_TOL * sse_r / cnt_r
    # raw x at the masked frames (-1 * s) would give a different number
    xr = torch.as_tensor(x, dtype=torch.float64)
    s, _ = R.model_forward(x, wt, K)
    raw = float((((xr * torch.as_tensor(s)) - torch.as_tensor(y, dtype=torch.float64)) ** 2).mean(-1).sum())
    assert abs(raw - sse_r) > 1e-3 * sse_r


def test_fit_with_reference_callbacks(dev, tmp_path):
    from drnmf_amd import callbacks as C
    B, T, F, H, K = 12, 8, 12, 10, 2
    rng = np.random.default_rng(21)
    x, y, w = _data(rng, B, T, F)
    xv, yv, wv = _data(rng, 5, T, F)
    m, _ = _model(dev, F, H, K, seed=5, lr=1e-3, clipnorm=1.0)
    hist_file, save_file = str(tmp_path / "hist.pkl"), str(tmp_path / "best.npz")
    ckpt = C.ModelCheckpoint(filepath=save_file, save_best_only=True, save_weights_only=True)
    hist = m.fit(x, y, sample_weight=w, batch_size=4, epochs=4, validation_data=(xv, yv, wv),
                 callbacks=[C.LossHistory(hist_file), ckpt, C.EarlyStopping(monitor="val_loss", patience=5)])
    assert len(hist["loss"]) == 4 and len(hist["val_loss"]) == 4
    with open(hist_file, "rb") as f:
        h = pickle.load(f)
    assert len(h["on_batch_end"]["loss"]) == 4 * 3 and len(h["on_epoch_end"]["val_loss"]) == 4
    best = int(np.argmin(hist["val_loss"]))
    m.load_weights(save_file)
    assert abs(float(m._validate((xv, yv, wv), 4, lambda a, b: a[b])) - hist["val_loss"][best]) <= \
        1e-5 * hist["val_loss"][best]


def test_determinism_graph_and_nan_workspace(dev, monkeypatch):
    B, T, F, H, K = 9, 14, 20, 24, 3
    rng = np.random.default_rng(30)
    x, y, w = _data(rng, B, T, F)
    runs = []
    for _ in range(2):
        m, _ = _model(dev, F, H, K, seed=13, lr=1e-3)
        for _ in range(3):
            m.train_on_batch(x, y, w)
        runs.append(m.get_weights())
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    m, _ = _model(dev, F, H, K, seed=13)
    _, _, g_graph = _grads(m, dev, x, y, w)
    monkeypatch.setenv("DRNMF_NO_GRAPH", "1")
    _, _, g_direct = _grads(m, dev, x, y, w)
    monkeypatch.delenv("DRNMF_NO_GRAPH")
    for a, b in zip(g_graph, g_direct):
        assert np.array_equal(a, b)
    m2, _ = _model(dev, F, H, K, seed=13)
    from drnmf_amd import _capi
    import ctypes
    need = _capi.lib().drnmf_lstm_train_workspace_bytes(ctypes.byref(m2._desc(B, T)))
    m2._train_ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=dev).view(torch.uint8)
    _, _, g_nan = _grads(m2, dev, x, y, w)
    for a, b in zip(g_graph, g_nan):
        assert np.array_equal(a, b)
