"""The LSTM baseline on the GPU (build_lstm, enhance.py:321-345; csrc/lstm.hip): hidden states and the sigmoid
output against the fp64 reference restatement (tests/lstm_ref.py), predict's slab loop, determinism.

Tolerance: max|d| / max|ref| <= 1e-4 (fp32 kernels vs fp64 reference), as for the other recurrent cells.
"""
import numpy as np
import pytest
import torch

import lstm_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (run with -m 'not gpu' on CPU boxes)")
    from drnmf_amd import _capi
    _capi.handle(0)
    return torch.device("cuda:0")


def _check(got, ref, what):
    scale = max(float(np.max(np.abs(ref))), 1e-30)
    err = float(np.max(np.abs(got - ref))) / scale
    assert err <= TOL, "%s: max|d|/max|ref| = %.3e" % (what, err)


def _model(dev, F, H, K, act="hard_sigmoid", seed=0, scale=1.0):
    from drnmf_amd import layers
    m = layers.build_lstm(dict(mask_value=-1., maxseq=8, input_dim=F, output_dim=F, K_layers=K, hidden_dim=H,
                               recurrent_activation=act), device=dev)
    w = R.random_weights(np.random.default_rng(seed), F, H, K, scale=scale)
    m.set_weights(w)
    return m, w


# (B, T, F, H, K): every shipped hidden size, K in {1, 2, 5}, B in {1, 3, 32, 250}, F in {513, small}, odd H
CASES = [(3, 17, 20, 13, 1), (1, 40, 513, 54, 2), (32, 30, 513, 54, 2), (3, 33, 33, 70, 5), (32, 25, 513, 70, 5),
         (1, 30, 513, 244, 2), (32, 40, 513, 250, 5), (250, 12, 513, 250, 5), (250, 20, 48, 37, 1)]


@pytest.mark.parametrize("act", ["hard_sigmoid", "sigmoid"])
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "B%dT%dF%dH%dK%d" % s)
def test_forward_matches_reference(dev, shape, act):
    B, T, F, H, K = shape
    rng = np.random.default_rng(B * 1000 + H)
    x, _ = R.ragged_input(rng, B, T, F)
    m, w = _model(dev, F, H, K, act, seed=H + K, scale=1.5)
    y, h = m.forward(torch.from_numpy(x).to(dev), want_hidden=True)
    torch.cuda.synchronize()
    y_ref, h_ref = R.model_forward(x, w, K, -1.0, act)
    _check(h.cpu().numpy(), h_ref, "hidden")
    _check(y.cpu().numpy(), y_ref, "output")
    if B > 1:                                  # the all-masked row: zero states, sigmoid(b_out) everywhere
        assert float(h[-1].abs().max()) == 0.0


def test_unmasked_input_and_hidden_of_every_frame(dev):
    """mask_value None: no frame is masked (the same path with every valid flag set)."""
    from drnmf_amd import ops
    B, T, F, H, K = 5, 21, 40, 24, 3
    rng = np.random.default_rng(7)
    w = R.random_weights(rng, F, H, K, scale=1.5)
    x = rng.standard_normal((B, T, F)).astype(np.float32)
    x[:, 3:5] = -1.0                            # would be masked frames: with mask_value None they are not
    desc = ops.make_lstm_desc(B, T, F, H, K)
    t = lambda a: torch.from_numpy(a).to(dev)
    p = ops.lstm_prepare_params(desc, [t(a) for a in w[0:3 * K:3]], [t(a) for a in w[1:3 * K:3]],
                                [t(a) for a in w[2:3 * K:3]], t(w[-2]), t(w[-1]))
    h = ops.lstm_forward(t(x), None, p, desc)
    ref = R.lstm_layers(x, w[0:3 * K:3], w[1:3 * K:3], w[2:3 * K:3], None, "hard_sigmoid")[-1].numpy()
    _check(h.cpu().numpy(), ref, "hidden")


def test_predict_slabs_and_length_aware_run(dev):
    """predict(batch_size=250) = per-slab predict_on_batch; the length-aware run = the padded run."""
    n, T, F, H, K = 260, 40, 513, 54, 2
    rng = np.random.default_rng(3)
    x, lens = R.ragged_input(rng, n, T, F)
    m, _ = _model(dev, F, H, K, scale=1.5)
    out = m.predict(x, batch_size=250)
    slabs = np.concatenate([m.predict_on_batch(x[:250]), m.predict_on_batch(x[250:])])
    padded = m.predict(x, batch_size=250, length_aware=False)
    np.testing.assert_allclose(out, slabs, rtol=0, atol=1e-6)
    np.testing.assert_allclose(out, padded, rtol=0, atol=1e-6)
    y_ref, _ = R.model_forward(x[:8], m.get_weights(), K)
    _check(out[:8], y_ref, "predict")


def test_repeated_calls_and_direct_launches_are_bit_identical(dev, monkeypatch):
    B, T, F, H, K = 32, 37, 513, 70, 5
    x, _ = R.ragged_input(np.random.default_rng(11), B, T, F)
    m, _ = _model(dev, F, H, K, scale=1.5)
    xd = torch.from_numpy(x).to(dev)
    a = m.forward(xd).cpu()
    b = m.forward(xd).cpu()
    monkeypatch.setenv("DRNMF_NO_GRAPH", "1")
    c = m.forward(xd).cpu()
    assert torch.equal(a, b) and torch.equal(a, c)


def test_weights_set_after_a_forward_are_used(dev):
    """The prepared block follows in-place weight changes (set_weights, load_weights)."""
    B, T, F, H, K = 3, 9, 20, 13, 2
    x, _ = R.ragged_input(np.random.default_rng(5), B, T, F)
    m, w = _model(dev, F, H, K)
    m.forward(torch.from_numpy(x).to(dev))
    w2 = R.random_weights(np.random.default_rng(99), F, H, K, scale=1.5)
    m.set_weights(w2)
    y = m.forward(torch.from_numpy(x).to(dev)).cpu().numpy()
    _check(y, R.model_forward(x, w2, K)[0], "output after set_weights")


def test_padded_hidden_rows_and_head_paths_agree(dev):
    """lstm_forward returns hidden rows padded to round_up(H, 4) with zero padding (the head's vectorised path);
    the head on that view equals the head on a contiguous copy (stride H, the unvectorised path)."""
    from drnmf_amd import ops
    B, T, F, H, K = 6, 19, 513, 250, 2
    x, _ = R.ragged_input(np.random.default_rng(21), B, T, F)
    m, w = _model(dev, F, H, K, scale=1.5)
    y, h = m.forward(torch.from_numpy(x).to(dev), want_hidden=True)
    ld = ops.lstm_hidden_ld(H)
    assert h.stride() == (T * ld, ld, 1)
    assert float(h.as_strided((B, T, ld), (T * ld, ld, 1))[..., H:].abs().max()) == 0.0
    desc = ops.make_lstm_desc(B, T, F, H, K)
    y2 = ops.lstm_head_forward(h.contiguous(), m._params(desc), desc)
    torch.cuda.synchronize()
    y_ref = R.model_forward(x, w, K)[0]
    _check(y.cpu().numpy(), y_ref, "head, padded rows")
    _check(y2.cpu().numpy(), y_ref, "head, contiguous rows")
