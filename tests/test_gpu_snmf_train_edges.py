"""The sparse-NMF dictionary-training kernels (csrc/snmf.hip: drnmf_snmf_train_init / drnmf_snmf_train_step) at the
shapes where they take another path, against the float64 reference of tests/snmf_train_ref.py and within its bounds
(8 x the float32 yardstick of the same reference: below 1/n, so that one dropped or doubled frame of a frame sum does
not fit).  tests/test_gpu_parity.py::test_snmf_training_matches_oracle stays the 25-iteration end-to-end check; the
cases here (snmf_train_ref.CASES) reach split-K counts 1, 2, 4, 5 and 21, 0..4 tail rows in both instances of the tail
kernel, one / two / three workgroup columns of the thread-per-atom kernels, and the step with the W update off.

Every check prints "SNMF-EDGE <test> <case> <rule values> <errors>" before it asserts.
"""
import ctypes

import numpy as np
import pytest
import torch

import snmf_train_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (run with -m 'not gpu' on CPU boxes)")
    from drnmf_amd import _capi
    _capi.handle(0)
    return torch.device("cuda:0")


@pytest.fixture
def f32(dev):
    """Matrix mode 'f32' for the test, the previous one restored afterwards."""
    from drnmf_amd import ops
    prev = ops.set_matrix_mode("f32", dev)
    yield
    ops.set_matrix_mode(prev, dev)


@pytest.fixture
def x3(dev):
    from drnmf_amd import ops
    prev = ops.set_matrix_mode("bf16x3", dev)
    yield
    ops.set_matrix_mode(prev, dev)


def _dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


_REFS = {}


def _reference(c, beta, steps, update_w=True, kind="case"):
    """(inputs, mask, float64 reference) per run, computed once and shared by the tests (never modified)."""
    kind = R.MASKS[c] if kind == "case" else kind
    key = (c, beta, steps, update_w, kind)
    if key not in _REFS:
        V, W0, H0 = R.problem(R.CASES[c], beta)
        m = R.w_ind(R.CASES[c][2], kind)
        _REFS[key] = ((V, W0, H0), m, R.step_reference(V, W0, H0, R.SPARSITY, steps, beta, m, update_w))
    return _REFS[key]


def _device_run(dev, inputs, beta, steps, mask, update_w=True):
    """`steps` iterations from a fresh ops.SnmfTrainer -> (W (F,N), H (N,n), div[], cost[]) as numpy, and the trainer."""
    from drnmf_amd import ops
    V, W0, H0 = inputs
    tr = ops.SnmfTrainer(_dv(V.T, dev), _dv(W0, dev), _dv(H0.T, dev), beta=beta)
    md = None if mask is None else torch.from_numpy(mask.astype(np.uint8)).to(dev)
    log = torch.zeros((steps, 2), dtype=torch.float32, device=dev)
    for i in range(steps):
        tr.step(R.SPARSITY, md, update_w, obj=log[i])
    torch.cuda.synchronize()
    o = log.cpu().numpy()
    return (tr.W.cpu().numpy(), tr.H.cpu().numpy().T, o[:, 0], o[:, 1]), tr


def _report(test, c, beta, what, errs):
    r = R.rules(R.CASES[c])
    print("SNMF-EDGE %s %s %s beta %g %s | %s | %s" % (test, c, R.CASES[c], beta, what,
                                                     " ".join("%s=%d" % kv for kv in r.items()), R.fmt(errs)))


def _check(test, c, beta, what, got, ref, widen=0.0):
    errs = R.errors(got, ref, R.CASES[c])
    _report(test, c, beta, what, errs)
    bad = R.over_bound(errs, widen)
    assert not bad, "case %s beta %g %s: %s" % (c, beta, what, "; ".join("%s: %.3e > %.1e" % b for b in bad))
    return errs


def _normalised(W0):
    W0 = W0.astype(np.float64)
    return W0 / np.sqrt((W0 * W0).sum(0))


def _check_w(c, got, inputs, mask):
    W = got[0].astype(np.float64)
    np.testing.assert_allclose((W * W).sum(0), 1.0, rtol=R.UNIT_NORM_TOL, err_msg="case %s: column norms" % c)
    if mask is not None and not mask.all():
        W0n = _normalised(inputs[1])
        err = np.max(np.abs(W[:, ~mask] - W0n[:, ~mask])) / np.max(np.abs(W0n[:, ~mask]))
        assert err <= R.W_BOUND, "case %s: frozen columns moved by %.3e" % (c, err)


_STEP_PARAMS = [(c, b) for c in R.CASES for b in R.betas_of(c)]


@pytest.mark.parametrize("c,beta", _STEP_PARAMS, ids=["%s-beta%g" % p for p in _STEP_PARAMS])
def test_step_against_the_reference(dev, f32, c, beta):
    """One and three iterations from a fresh trainer: W (whole and by region), H, div and cost within the bounds, unit
    column norms, frozen columns equal to the normalised W0."""
    for steps in (1, 3):
        inputs, mask, ref = _reference(c, beta, steps)
        got, _ = _device_run(dev, inputs, beta, steps, mask)
        assert all(np.isfinite(a).all() for a in got)
        _check("step", c, beta, "steps %d mask %s" % (steps, R.MASKS[c]), got, ref)
        _check_w(c, got, inputs, mask)


@pytest.mark.parametrize("beta", [2.0, 1.0])
@pytest.mark.parametrize("c", R.H_ONLY)
def test_h_only_step(dev, f32, c, beta):
    """update_w = 0: H and both objective entries within the bounds, W never written, and the mask ignored."""
    inputs, _, ref = _reference(c, beta, 3, update_w=False)
    from drnmf_amd import ops
    probe = ops.SnmfTrainer(_dv(inputs[0].T, dev), _dv(inputs[1], dev), _dv(inputs[2].T, dev), beta=beta)
    torch.cuda.synchronize()
    W_init = probe.W.clone()
    got, tr = _device_run(dev, inputs, beta, 3, None, update_w=False)
    _check("h_only", c, beta, "steps 3 mask None", got, ref)
    assert torch.equal(tr.W, W_init), "case %s: W was written with update_w = 0" % c
    ones = np.ones(R.CASES[c][2], bool)
    got1, tr1 = _device_run(dev, inputs, beta, 3, ones, update_w=False)
    for name, a, b in zip(("W", "H", "div", "cost"), got, got1):
        assert np.array_equal(a, b), "case %s: %s differs between mask None and a mask of ones" % (c, name)
    assert torch.equal(tr1.W, W_init)


@pytest.mark.parametrize("cf,beta", [("ed", 2.0), ("kl", 1.0)])
def test_host_entry_with_nothing_to_update(dev, f32, cf, beta):
    """snmf.sparse_nmf with w_update_ind all false takes the update_w = 0 step: same bounds, W = the normalised init_w."""
    from drnmf_amd import snmf
    c = "C"
    inputs, _, ref = _reference(c, beta, 3, update_w=False, kind="none")
    V, W0, H0 = inputs
    params = dict(cf=cf, sparsity=R.SPARSITY, max_iter=3, conv_eps=0.0, init_w=W0, init_h=H0,
                  w_update_ind=R.w_ind(R.CASES[c][2], "none"))
    W, H, obj = snmf.sparse_nmf(V, params, device=dev)
    assert len(obj["cost"]) == 3 and len(obj["div"]) == 3
    _check("host_entry", c, beta, "cf %s" % cf, (W, H, obj["div"], obj["cost"]), ref)
    np.testing.assert_allclose(W, _normalised(W0), rtol=0, atol=R.W_BOUND * np.max(_normalised(W0)))


@pytest.mark.parametrize("beta", [2.0, 1.0])
@pytest.mark.parametrize("c", ["B", "D"])
def test_split_operand_mode_on_the_shared_kernels(dev, x3, c, beta):
    """The split-operand matrix mode shares every kernel named above but the products themselves: the same checks,
    each bound widened by the project's mode-to-mode bar."""
    inputs, mask, ref = _reference(c, beta, 3)
    got, _ = _device_run(dev, inputs, beta, 3, mask)
    _check("bf16x3", c, beta, "steps 3 mask %s" % R.MASKS[c], got, ref, widen=R.MODE_TOL)
    _check_w(c, got, inputs, mask)


def _capi_run(dev, inputs, beta, steps, fill, short=0):
    """drnmf_snmf_train_init + `steps` x _step through the C ABI on a workspace of the test's, filled with `fill`
    first.  short: bytes taken off the size that is PASSED (the buffer keeps its size).  -> rc of init, rc of the
    steps, W, H, log."""
    from drnmf_amd import _capi
    L, h = _capi.lib(), _capi.handle(0)
    V, W0, H0 = inputs
    Vd, W, H = _dv(V.T, dev), _dv(W0, dev), _dv(H0.T, dev)
    n, F = Vd.shape
    N = W.shape[1]
    nbytes = L.drnmf_snmf_train_workspace_bytes(n, F, N)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.full((nbytes // 4,), fill, dtype=torch.float32, device=dev)
    log = torch.zeros((steps, 2), dtype=torch.float32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc0 = L.drnmf_snmf_train_init(h, n, F, N, beta, _capi.ptr(Vd), _capi.ptr(W), _capi.ptr(H), _capi.ptr(ws),
                                  nbytes - short, stream)
    rcs = [L.drnmf_snmf_train_step(h, n, F, N, beta, R.SPARSITY, _capi.ptr(W), _capi.ptr(H), None, 1,
                                   _capi.ptr(log[i]), _capi.ptr(ws), nbytes - short, stream) for i in range(steps)]
    torch.cuda.synchronize()
    return rc0, rcs, W, H, log


@pytest.mark.parametrize("beta", [2.0, 1.0])
@pytest.mark.parametrize("c", ["B", "C", "F"])
def test_results_do_not_depend_on_the_workspace(dev, f32, c, beta):
    """What init and step never write -- the padded rows F..Fp4 of the partial buffers, the bins w_fold_kernel
    re-reads to add +0, the tail rows j >= ntail the reduce kernel skips, the unused half of the objective partials
    -- must not reach a result: a workspace of NaN and one of zeros give the same finite bits."""
    inputs = R.problem(R.CASES[c], beta)
    res = {}
    for fill in (float("nan"), 0.0):
        rc0, rcs, W, H, log = _capi_run(dev, inputs, beta, 2, fill)
        assert rc0 == 0 and rcs == [0, 0]
        assert all(bool(torch.isfinite(t).all()) for t in (W, H, log)), "case %s beta %g fill %r" % (c, beta, fill)
        res[fill == 0.0] = (W, H, log)
    print("SNMF-EDGE workspace %s %s beta %g | %s" % (c, R.CASES[c], beta,
                                                    " ".join("%s=%d" % kv for kv in R.rules(R.CASES[c]).items())))
    for name, a, b in zip(("W", "H", "objective"), res[False], res[True]):
        assert torch.equal(a, b), "case %s beta %g: %s depends on what the workspace held" % (c, beta, name)


def test_workspace_refusals(dev):
    """One byte short is DRNMF_ERR_WORKSPACE from both entry points, W and H untouched; the size grows with n."""
    from drnmf_amd import _capi
    inputs = R.problem(R.CASES["C"], 2.0)
    rc0, rcs, W, H, log = _capi_run(dev, inputs, 2.0, 1, 0.0, short=1)
    assert rc0 == -4 and rcs == [-4]                                       # include/drnmf.h DRNMF_ERR_WORKSPACE
    assert torch.equal(W, _dv(inputs[1], dev)) and torch.equal(H, _dv(inputs[2].T, dev))
    assert float(log.abs().sum()) == 0.0
    L = _capi.lib()
    ns = sorted(set(s[0] for s in R.CASES.values()))
    for _, F, N in R.CASES.values():
        sizes = [L.drnmf_snmf_train_workspace_bytes(n, F, N) for n in ns]
        assert all(a > 0 and a <= b for a, b in zip(sizes, sizes[1:])), (F, N, sizes)


@pytest.mark.parametrize("c", ["B", "D"])
def test_two_runs_give_the_same_bits(dev, f32, c):
    """Fixed summation orders throughout: two fresh trainers, three steps each, the same bits."""
    inputs, mask, _ = _reference(c, 1.0, 3)
    a, _ = _device_run(dev, inputs, 1.0, 3, mask)
    b, _ = _device_run(dev, inputs, 1.0, 3, mask)
    for name, x, y in zip(("W", "H", "div", "cost"), a, b):
        assert np.array_equal(x, y), "case %s: %s differs between two runs" % (c, name)
