"""Relu sign bits of the training forward (csrc/cell_shared.h, relu_bits_*): cell_a records one bit per
stored hidden, bwd_a / bwd_edge read the bits instead of the stored hiddens.  The bits ARE the comparison
the kernels made before, so every gradient must be bit-identical with DRNMF_RELU_BITS=1 and =0 -- checked
with numpy.array_equal on the whole flat buffer of loss_and_grads (loss and counts included) and on
d_log_h0 -- and, like before, within tests/test_gpu_train.py's tolerance of fp64 autograd.

Shapes: the smallest at which each part can go wrong -- a partly live last atom block (N = 14, 40), dead
workgroups past the last atom block (N = 260: 9 blocks in a grid of 16), a partly filled row tile (B = 3,
18), with and without the odd bin (F = 33, 21), the edge kernel alone (K = 1), K = 2 and 3, T = 5, ragged
lengths with an interior masked frame and a row with no valid frame, tied and untied layers, a stateful
layer over two batches.

Which path a call took is probed through the cell's own two halves: the BPTT is run once more on a copy of
the stored hiddens whose zeros are 1e-30 -- nothing to any product that uses the VALUES, but [h > 0] turns
true wherever it was false.  Where the bits are read the gradients do not move; where the stored hiddens
are read (DRNMF_RELU_BITS=0, the Gram form, fp16 operands) they do."""
import numpy as np
import pytest
import torch

from oracle import drnmf_oracle as O
from test_gpu_train import G_TOL, _autograd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from drnmf_amd import _capi
    _capi.handle(0)
    return torch.device("cuda:0")


def _problem(B, T, F, r, seed):
    P = O.synth_problem(B, T, F, r, seed=seed, ragged=True, density=0.15)
    P["X"][0, 1] = -1.0                   # an interior masked frame in a row that goes on
    P["Y"][0, 1] = -1.0
    P["X"][B - 1] = -1.0                  # a row with no valid frame
    P["Y"][B - 1] = -1.0
    P["X"][1, :] = np.where(P["X"][1, :] == -1.0, 0.5, P["X"][1, :])      # a row of full length
    P["Y"][1, :] = np.where(P["Y"][1, :] == -1.0, 0.5, P["Y"][1, :])
    return P


def _model(P, F, r, K, untied, T, seed, operand_dtype="float32", stateful=False, alph=None, lam1=0.3):
    from drnmf_amd import layers
    np.random.seed(seed)                  # log_h0's 'uniform' initialiser draws from the global generator
    N = 2 * r
    p = dict(input_dim=F, hidden_dim=N, output_dim=F, mask_value=-1., maxseq=T, K_layers=K, W=P["W"],
             alph=N / 4.0 if alph is None else alph, lam1=lam1, params_untied=list(untied),
             params_trainable=["log_D", "log_alph"], operand_dtype=operand_dtype)
    model = layers.build_unfolded_snmf(p)
    rng = np.random.default_rng(seed)
    w = model.get_weights()
    w = [a + (0.05 * rng.standard_normal(a.shape)).astype(np.float32)
         if (a.ndim == 2 and a.shape[0] != a.shape[1]) or a.ndim == 1 else a for a in w]
    model.set_weights(w)
    model.cell.stateful = stateful
    model.compile(lr=1e-3)
    return model


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _wmask(P):
    return (P["X"] != -1.0).any(-1).astype(np.float32)


def _grads(model, batches, dev):
    """[(flat buffer, d_log_h0)] of loss_and_grads over consecutive batches."""
    res = []
    for P in batches:
        flat = model.loss_and_grads(_t(P["X"], dev), _t(P["Y"], dev), _t(_wmask(P), dev))
        torch.cuda.synchronize()
        res.append((flat.cpu().numpy().copy(), model._gview["log_h0"].cpu().numpy().copy()))
    return res


def _reads_stored_hiddens(model, P, dev):
    """True when the BPTT of this model's cell takes its relu masks from the stored hiddens, False when it
    takes them from the recorded bits (see the module docstring)."""
    cell = model.cell
    x = _t(P["X"], dev)
    hall = cell.forward_train(x, -1.0)
    N = hall.shape[-1] // cell.K_layers
    gen = torch.Generator(device="cpu").manual_seed(3)
    d_out = torch.rand((x.shape[0], x.shape[1], N), generator=gen).to(dev)
    keys = ("d_log_D", "d_log_alph", "d_log_h0")
    g0 = {k: v.clone() for k, v in cell.backward(x, hall, d_out).items() if k in keys}
    hall_p = torch.where(hall == 0, torch.full_like(hall, 1e-30), hall)
    # (the probe, and the case itself, mean something only where valid frames hold zeros AND positive values)
    live = _t(_wmask(P), dev)[:, :, None] > 0
    assert bool(((hall == 0) & live).any()) and bool(((hall > 0) & live).any())
    g1 = {k: v.clone() for k, v in cell.backward(x, hall_p, d_out).items() if k in keys}
    torch.cuda.synchronize()
    moved = []
    for k in keys:
        a, b = g0[k].cpu().numpy().astype(np.float64), g1[k].cpu().numpy().astype(np.float64)
        moved.append(np.max(np.abs(a - b)) / max(np.max(np.abs(a)), 1e-30))
    # (bits: the values 1e-30 change nothing an fp32 sum can hold; stored hiddens: whole rows of dz appear)
    assert max(moved) <= 1e-6 or max(moved) >= 1e-3, moved
    return max(moved) >= 1e-3


def _check_autograd(model, P, K, got, initial_state=None):
    flat, _ = got
    ref_loss, ref, cnt = _autograd(model, P, _wmask(P), K, False, initial_state=initial_state)
    assert abs(float(flat[-4]) - ref_loss) <= 1e-5 * abs(ref_loss) + 1e-9
    assert float(flat[-3]) == cnt
    name_map = {"kernel_clean": "kc", "kernel_noise": "kn"}
    o = 0
    for n, t in model._train_items:
        g = flat[o:o + t.numel()].reshape(tuple(t.shape))
        o += t.numel()
        if initial_state is not None and n == "log_h0":
            assert not g.any()
            continue
        r_ = ref[name_map.get(n, n)]
        err = np.max(np.abs(g - r_)) / max(np.max(np.abs(r_)), 1e-12)
        assert err <= G_TOL, "%s: rel err %.3e" % (n, err)


CASES = [
    # one atom block, partly live; partly filled row tile; odd bin; untied
    dict(B=3, T=5, F=33, r=7, K=3, untied=("log_D", "log_alph")),
    # two atom blocks, the second partly live; two row tiles, the second partly filled; no odd bin; tied
    dict(B=18, T=5, F=21, r=20, K=2, untied=()),
    # the edge kernel alone, 9 atom blocks in a grid of 16: dead workgroups
    # (a large threshold: with lam1 = 0.3 one layer from softplus(log_h0) leaves every hidden positive;
    # 50 zeroes 38 % of them, 20 in the three-layer case below 6 %, and fp32 autograd stays within 3e-6 of fp64)
    dict(B=3, T=5, F=33, r=130, K=1, untied=(), lam1=50.0),
    # dead workgroups in bwd_a, two row tiles, untied, no odd bin
    dict(B=18, T=5, F=21, r=130, K=3, untied=("log_D", "log_alph"), lam1=20.0),
    # tied, odd bin, K = 2
    dict(B=3, T=5, F=33, r=20, K=2, untied=()),
]


@pytest.mark.parametrize("cfg", CASES)
def test_gradients_are_bit_identical_with_and_without_the_bits(dev, monkeypatch, cfg):
    monkeypatch.setenv("DRNMF_GRAM", "0")
    B, T, F, r, K = (cfg[k] for k in "BTFrK")
    P = _problem(B, T, F, r, seed=11)
    got = {}
    for bits in ("1", "0"):
        monkeypatch.setenv("DRNMF_RELU_BITS", bits)
        model = _model(P, F, r, K, cfg["untied"], T, seed=11, alph=cfg.get("alph"), lam1=cfg.get("lam1", 0.3))
        got[bits] = _grads(model, [P], dev)[0]
        assert _reads_stored_hiddens(model, P, dev) == (bits == "0")
    assert np.array_equal(got["1"][0], got["0"][0])
    assert np.array_equal(got["1"][1], got["0"][1])
    assert np.isfinite(got["1"][0]).all() and got["1"][0][:-4].any()
    _check_autograd(model, P, K, got["1"])


def test_stateful_layer_over_two_batches(dev, monkeypatch):
    monkeypatch.setenv("DRNMF_GRAM", "0")
    B, T, F, r, K = 3, 5, 33, 7, 2
    P1, P2 = _problem(B, T, F, r, seed=11), _problem(B, T, F, r, seed=12)
    P2["W"] = P1["W"]
    got = {}
    for bits in ("1", "0"):
        monkeypatch.setenv("DRNMF_RELU_BITS", bits)
        model = _model(P1, F, r, K, ("log_D", "log_alph"), T, seed=11, stateful=True)
        got[bits] = _grads(model, [P1, P2], dev)
    for a, b in zip(got["1"], got["0"]):
        assert np.array_equal(a[0], b[0])
        assert np.array_equal(a[1], b[1])
    # fp64 autograd from the same entering states: zeros, then what the first batch left
    names = ["log_h0"] + list(model.cell._alt.keys()) + ["kc", "kn"]
    wd = dict(zip(names, model.get_weights()))
    alt = {k: wd[k] for k in model.cell._alt.keys()}
    labels = model.cell.maps_from_alt.labels_per_k
    state = np.zeros((B, 2 * r), np.float64)
    for Pb, g in zip((P1, P2), got["1"]):
        _check_autograd(model, Pb, K, g, initial_state=state)
        _, state = O.cell_forward_factored(Pb["X"], O.maps_factored(alt, labels, K), O.u_scalars(alt),
                                           wd["log_h0"], mask_value=-1.0, initial_state=state, return_state=True)


@pytest.mark.parametrize("form", ["gram", "f16"])
def test_forms_without_bits_keep_reading_the_stored_hiddens(dev, monkeypatch, form):
    """The Gram form (forced) and the fp16-operand forward record no bits: their BPTT reads the stored hiddens
    whatever DRNMF_RELU_BITS says, and is as right as before."""
    monkeypatch.setenv("DRNMF_GRAM", "1" if form == "gram" else "0")
    B, T, F, r, K = 3, 5, 33, 7, 3
    P = _problem(B, T, F, r, seed=11)
    got = {}
    for bits in ("1", "0"):
        monkeypatch.setenv("DRNMF_RELU_BITS", bits)
        model = _model(P, F, r, K, ("log_D", "log_alph"), T, seed=11,
                       operand_dtype="float16" if form == "f16" else "float32")
        got[bits] = _grads(model, [P], dev)[0]
        assert _reads_stored_hiddens(model, P, dev)
    assert np.array_equal(got["1"][0], got["0"][0])
    assert np.array_equal(got["1"][1], got["0"][1])
    if form == "gram":
        _check_autograd(model, P, K, got["1"])
    else:
        # fp16 operands in the forward: within fp16-rounding distance of the exact model's fp64 autograd
        # (the bound of test_mixed_precision_training_fp16_forward_fp32_bptt)
        model32 = _model(P, F, r, K, ("log_D", "log_alph"), T, seed=11)
        _, ref, _ = _autograd(model32, P, _wmask(P), K, False)
        o = 0
        for n, t in model._train_items:
            g = got["1"][0][o:o + t.numel()].reshape(tuple(t.shape))
            o += t.numel()
            r_ = ref[{"kernel_clean": "kc", "kernel_noise": "kn"}.get(n, n)]
            assert np.max(np.abs(g - r_)) / max(np.max(np.abs(r_)), 1e-30) <= 3e-2, n
