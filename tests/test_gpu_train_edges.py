"""The DR-NMF training kernels (csrc/cell_backward.hip: BPTT chain, time-batched weight gradients, column sums,
parameter maps; csrc/train.hip: the two loss heads) one stage at a time and at the shapes where they take another
path, against the fp64 references of tests/drnmf_train_ref.py.  tests/test_gpu_train.py checks the same kernels end
to end; this is the counterpart of tests/test_gpu_lstm_train_edges.py for the product's own cell.

  A  split-K weight gradients (gemm_tn with 1, 2, 8 splits, an empty trailing split, a partial last k-tile), the
     256-split column reduction in its three instances and two folds, the three forms of the d log_D map: dense
     cotangents, ONE live frame (so that a lost row is the whole gradient, not 0.1 % of it), poisoned memory, KL/beta;
  B  the two loss heads alone on a hidden tensor of the test's choosing;
  C  the BPTT alone on cotangents no loss head produces;
  D  lengths across the frames-per-graph boundary, replayed twice and against direct launches;
  E  one dimension at a time across the tiles, the row-blocked and atom-range instances, qred, odd N through ops.*;
  F  mask_value 0.0.

Bounds: G_TOL (max|d| / max|ref|) and the loss bound of tests/test_gpu_train.py, counts exact.  One-frame cases are
normalised by the whole tensor, dense cases additionally per slice (d log_D per stored layer, MFMA bins and tail rows
apart; d log_alph per stored layer; d log_lam1 over the layers).  A ReLU within fp32 rounding of 0 can take the other
side on the device, where its derivative differs by 1: every max-bounded case first asserts
drnmf_train_ref.relu_margin >= H_TOL over the rows that carry cotangent (a condition on the INPUT, from the fp64 run
alone; SEEDS were picked for it).  Cases with too many activations for that (the dense long ones of A and D, qred)
use the form test_gradients_match_autograd uses for its large case -- at most 1e-3 of the elements off by more than
G_TOL, relative L2 error <= G_TOL -- per slice, after asserting that fp32 CPU autograd of the same graph stays
inside that cap; each is paired with one-frame cases at the same shape under the plain bound.

Every check prints "EDGE <group> <mode> <case> <array/slice> <error>" before it asserts.
"""
import numpy as np
import pytest
import torch

import drnmf_train_ref as R
from oracle import drnmf_torch_ref as TR
from test_gpu_lstm_train_edges import _matrix_mode
from test_gpu_parity import H_TOL
from test_gpu_train import G_TOL, _setup

pytestmark = pytest.mark.gpu

L_TOL = 1e-5
FORMS = pytest.mark.parametrize("cell_form", ["auto", "factored"], indirect=True)
FACTORED = pytest.mark.parametrize("cell_form", ["factored"], indirect=True)

# seeds of _setup (synthetic batch, initialisers, weight perturbation), picked on the CPU so that the case's
# precondition holds (relu_margin >= H_TOL, or fp32 CPU autograd inside the outlier cap); every other case: 5
SEEDS = {("A", "A4a"): 1, ("A", "A4b"): 6, ("A5", 65): 1, ("C", "untie_alph"): 1, ("F", 0.0): 1, ("E", "qred"): 8,
         ("E", (15, 4, 33, 8, 3)): 6, ("E", (16, 4, 33, 8, 3)): 3, ("E", (17, 4, 33, 8, 3)): 8,
         ("E", (33, 4, 33, 8, 3)): 6, ("E", (3, 4, 33, 15, 3)): 1, ("E", (3, 4, 33, 17, 3)): 1,
         ("E", (3, 4, 33, 33, 3)): 1, ("E", (3, 4, 31, 8, 3)): 1, ("E", (3, 4, 48, 8, 3)): 2,
         ("E", (3, 4, 33, 65, 3)): 3, ("E", (3, 4, 33, 130, 3)): 22, ("E", (3, 4, 33, 170, 3)): 3}


def _seed(*key):
    return SEEDS.get(key, 5)


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
    with _matrix_mode(request.param, dev) as m:
        yield m


def _dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


_REFS = {}


def _cached(key, fn):
    """One reference per case, shared by the matrix modes and cell forms (and never modified)."""
    if key not in _REFS:
        _REFS[key] = fn()
    return _REFS[key]


# ---- the cell under test and its reference ---------------------------------------------------------------------

ARRAYS = ("d_log_D", "d_log_alph", "d_log_lam1", "d_log_h0")


def _stack(g, labels):
    """{alt name: gradient} -> the arrays of ops.cell_backward: one slot per STORED layer."""
    uniq = lambda name: list(dict.fromkeys(labels[name]))
    return {"d_log_D": np.stack([g[n] for n in uniq("log_D")]),
            "d_log_alph": np.stack([np.asarray(g[n]).reshape(-1) for n in uniq("log_alph")]),
            "d_log_lam1": np.stack([np.asarray(g[n]).reshape(()) for n in uniq("log_lam1")]),
            "d_log_h0": g["log_h0"]}


class Cell(object):
    """A model of tests/test_gpu_train._setup; its cell's training forward + BPTT on a cotangent of the caller's."""

    def __init__(self, dev, B, T, F, r, K, untied=("log_D", "log_alph"), untie_alph=False, seed=5, divergence="ed",
                 beta=1.5):
        self.dev, self.shape, self.K, self.F, self.N = dev, (B, T, F, r, K), K, F, 2 * r
        self.model, P, _ = _setup(B, T, F, r, K, untied, untie_alph=untie_alph, seed=seed,
                                  trainable=("log_D", "log_alph", "log_lam1"), divergence=divergence, beta=beta)
        self.x0 = P["X"]
        cell = self.model.cell
        wd = dict(zip(["log_h0"] + list(cell._alt.keys()) + ["kc", "kn"], self.model.get_weights()))
        self.alt = {k: wd[k] for k in cell._alt.keys()}
        self.log_h0 = wd["log_h0"]
        self.labels = cell.maps_from_alt.labels_per_k
        self.div = dict(divergence=divergence, beta=beta)

    def vjp(self, x, cot, mask_value=-1.0, state=None):
        cell = self.model.cell
        xd = _dv(x, self.dev)
        if state is not None:
            cell.stateful = True
            cell.states = [_dv(state, self.dev)]
        hall = cell.forward_train(xd, mask_value=mask_value)
        g = cell.backward(xd, hall, _dv(cot, self.dev))
        torch.cuda.synchronize()
        return {k: g[k].detach().cpu().numpy().astype(np.float64) for k in ARRAYS}

    def ref(self, x, cot, mask_value=-1.0, state=None, dtype=torch.float64):
        return _stack(R.cell_vjp(x, self.alt, self.labels, self.K, self.log_h0, cot, mask_value, state, dtype=dtype,
                                 **self.div), self.labels)

    def margin(self, x, rows=None, mask_value=-1.0, state=None):
        return R.relu_margin(x, self.alt, self.labels, self.K, self.log_h0, rows, mask_value, state, **self.div)

    def hidden(self, x, mask_value=-1.0):
        """The fp64 outputs [B,T,N] (which frames are valid, which atoms are alive)."""
        t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
        with torch.no_grad():
            return TR.cell_outputs(t(x), {k: t(v) for k, v in self.alt.items()}, self.labels, self.K,
                                   t(self.log_h0), mask_value, **self.div).numpy()


def _fill_row(x, b):
    """Row b fully valid: its masked tail repeats its valid frames."""
    L = int((x[b] != -1.0).any(-1).sum())
    assert L > 0
    for t in range(L, x.shape[1]):
        x[b, t] = x[b, t % L]
    return x


def _one_frame_input(cell, b, t):
    """Frames 0 .. t-1 of row b masked, frame t valid and with live atoms in the last layer: its own content where
    that is so, otherwise that of the row's frame with the most (entered from the initial state, as frame t is)."""
    x0 = cell.x0
    cand = x0[b][(x0[b] != -1.0).any(-1)]
    live = (cell.hidden(cand[:, None, :])[:, 0] > 0).sum(-1)
    assert live.max() >= 2
    x = x0.copy()
    if not (x[b, t] != -1.0).any() or (cell.hidden(x[b:b + 1, t:t + 1]) > 0).sum() < 2:
        x[b, t] = cand[int(np.argmax(live))]
    x[b, :t] = -1.0
    return x


# ---- checks ----------------------------------------------------------------------------------------------------

def _rel(got, ref):
    return float(np.max(np.abs(got - ref))) / max(float(np.max(np.abs(ref))), 1e-30)


def _slices(F, ref, divergence="ed"):
    """[(name, array, index)] of the per-slice bound."""
    nmain = 16 * R.nft_main_of(F, divergence) if R.ntail_of(F, divergence) else F
    out = []
    for k in range(ref["d_log_D"].shape[0]):
        out.append(("d_log_D[%d][mfma-bins]" % k, "d_log_D", (k, slice(0, nmain))))
        if nmain < F:
            out.append(("d_log_D[%d][tail-rows]" % k, "d_log_D", (k, slice(nmain, F))))
    out += [("d_log_alph[%d]" % k, "d_log_alph", (k,)) for k in range(ref["d_log_alph"].shape[0])]
    out += [("d_log_lam1", "d_log_lam1", ()), ("d_log_h0", "d_log_h0", ())]
    return out


def _whole(F, ref, divergence="ed"):
    return [(a, a, ()) for a in ARRAYS]


def _check_max(tag, got, ref, F, slices=_slices, divergence="ed", fail=None):
    """max|d| / max|ref| per slice: all printed, then all asserted (or collected in `fail`)."""
    errs = [(n, _rel(got[a][i], ref[a][i])) for n, a, i in slices(F, ref, divergence)]
    for n, e in errs:
        print("EDGE %s %s %.3e" % (tag, n, e))
    bad = ["%s %s: max|d|/max|ref| = %.3e" % (tag, n, e) for n, e in errs if not e <= G_TOL]
    if fail is not None:
        fail += bad
    else:
        assert not bad, "\n".join(bad)


def _outlier_figures(got, ref, F, divergence="ed"):
    out = []
    for n, a, i in _slices(F, ref, divergence):
        g, r_ = np.asarray(got[a][i]), np.asarray(ref[a][i])
        scale = max(float(np.max(np.abs(r_))), 1e-30)
        share = float(np.mean(np.abs(g - r_) > G_TOL * scale))
        l2 = float(np.linalg.norm(g - r_)) / max(float(np.linalg.norm(r_)), 1e-30)
        out.append((n, share, l2))
    return out


def _check_outliers(tag, got, ref, F, divergence="ed"):
    """The large-case form of test_gradients_match_autograd, per slice: at most 1e-3 of the elements off by more
    than G_TOL of the slice's maximum, relative L2 error <= G_TOL."""
    figs = _outlier_figures(got, ref, F, divergence)
    for n, share, l2 in figs:
        print("EDGE %s %s share=%.3e l2=%.3e" % (tag, n, share, l2))
    bad = ["%s %s: share %.3e, rel L2 %.3e" % (tag, n, s, l) for n, s, l in figs if not (s <= 1e-3 and l <= G_TOL)]
    assert not bad, "\n".join(bad)


def _assert_fp32_inside_cap(tag, ref32, ref, F, divergence="ed"):
    bad = [(n, s, l) for n, s, l in _outlier_figures(ref32, ref, F, divergence) if not (s <= 1e-3 and l <= G_TOL)]
    assert not bad, "%s: precondition -- fp32 CPU autograd itself leaves the cap: %r" % (tag, bad)


def _assert_margin(tag, m):
    assert m >= H_TOL, "%s: precondition -- a pre-activation of the fp64 run lies %.2e max|h| from 0" % (tag, m)


def _assert_zero(tag, got):
    for a in ARRAYS:
        print("EDGE %s %s %.3e" % (tag, a, float(np.max(np.abs(got[a])))))
    for a in ARRAYS:
        assert not got[a].any(), "%s %s: not exactly zero" % (tag, a)


def _one_frame(cell, tag, b, t, fail, group_key):
    """The one-frame construction at (b, t); the reference is that row alone, up to frame t."""
    B, T, F, r, K = cell.shape
    x = _cached(group_key + (b, t, 'x'), lambda: _one_frame_input(cell, b, t))
    cot = np.zeros((B, T, cell.N), np.float32)
    cot[b, t] = np.random.default_rng(1000 * b + t).standard_normal(cell.N)

    def ref():
        xs, cs = x[b:b + 1, :t + 1], cot[b:b + 1, :t + 1]
        _assert_margin(tag, cell.margin(xs))
        g = cell.ref(xs, cs)
        assert all(np.abs(g[a]).max() > 0 for a in ARRAYS), tag + ": the live frame must reach every gradient"
        return g
    _check_max(tag, cell.vjp(x, cot), _cached(group_key + (b, t), ref), F, _whole, cell.div["divergence"], fail)


# ---- A: time-batched weight gradients and column sums (both modes, both forms) ---------------------------------

# name -> (B, T, F, r, K), then BY HAND from the headers: (splits of the weight-gradient products, empty splits,
# colreduce instance, fold lanes, d log_D form)
A_SHAPES = {
    "A1": ((7, 220, 33, 6, 2), (8, [7], (4, 4, 4), 4, ("vec", 1, 9))),      # 49 k-tiles, 7 per split, last: 4 rows
    "A2": ((2, 207, 33, 6, 2), (2, [], (4, 4, 4), 4, ("vec", 1, 9))),       # 13 k-tiles, 7 + 6, last: 30 rows
    "A2c": ((2, 151, 33, 6, 2), (1, [], (4, 4, 4), 4, ("vec", 1, 9))),      # control: one split
    "A3": ((7, 220, 33, 7, 2), (8, [7], (1, 1, 8), 4, ("scalar", 0, 0))),   # N = 14: scalar gemm_tn, dlogd_kernel
    "A4a": ((2, 193, 33, 130, 2), (2, [], (4, 1, 4), 4, ("vec", 1, 9))),    # N = 260
    "A4b": ((2, 193, 33, 258, 2), (2, [], (4, 1, 4), 1, ("vec", 1, 9))),    # N = 516: one-lane fold
}


def _assert_a_plan(name, divergence="ed"):
    (B, T, F, r, K), want = A_SHAPES[name]
    N = 2 * r
    plan = R.tn_plan(R.bptt_gemm_m(F, divergence), N, B * T) + (R.colreduce_form(N), R.fold_form(N), R.dlogd_form(F, N))
    assert plan == want, "precondition: %s was chosen for the plan %r, the rules now give %r" % (name, want, plan)
    return plan


def _positions(B, T, splits):
    """name -> contraction row bt = b T + t of the one-frame cases."""
    BT = B * T
    nkt = (BT + 31) // 32
    per = (nkt + splits - 1) // splits * 32
    pos = {"first": 0, "seq0-last": T - 1, "seq1-first": T, "last": BT - 1}
    if splits > 1:
        pos.update({"split0-last": per - 1, "split1-first": per})
    if BT % 32:
        pos.update({"fullkt-last": BT // 32 * 32 - 1, "partial-first": BT // 32 * 32})
    return pos


@FORMS
@pytest.mark.parametrize("name", sorted(A_SHAPES))
def test_a_one_frame(dev, mode, cell_form, name):
    """ONE live frame at the first and last row, either side of the split boundary, either side of the partial
    k-tile and either side of the sequence boundary (which lies inside a column-reduction split that began in
    sequence 0): all of d log_D, d log_alph, d log_lam1, d log_h0 is that row's contribution."""
    (B, T, F, r, K), _ = A_SHAPES[name]
    splits = _assert_a_plan(name)[0]
    pos = _positions(B, T, splits)
    if name == "A1":
        assert pos == {"first": 0, "seq0-last": 219, "seq1-first": 220, "last": 1539, "split0-last": 223,
                       "split1-first": 224, "fullkt-last": 1535, "partial-first": 1536}
        assert R.cr_split_rows(R.cr_split_of(220, B * T), B * T) == (217, 224)
    r0, r1 = R.cr_split_rows(R.cr_split_of(T, B * T), B * T)
    assert r0 < T < r1                                   # bt = T inside a split that began in sequence 0
    cell = Cell(dev, B, T, F, r, K, untied=("log_D", "log_alph", "log_lam1"), seed=_seed("A", name))
    fail = []
    for pname, bt in sorted(pos.items(), key=lambda kv: kv[1]):
        _one_frame(cell, "A %s %s/%s one-frame-%s(bt=%d)" % (mode, name, cell_form, pname, bt), bt // T, bt % T,
                   fail, ("A1f", name))
    assert not fail, "\n".join(fail)


def _dense_input(cell, rng):
    B, T = cell.shape[:2]
    x = _fill_row(cell.x0.copy(), B - 1)                 # the last k-tiles and splits hold live frames
    return x, rng.standard_normal((B, T, cell.N)).astype(np.float32)


def _dense_outlier_case(cell, tag, key):
    x, cot = _dense_input(cell, np.random.default_rng(7))
    F = cell.F
    div = cell.div["divergence"]

    def ref():
        g = cell.ref(x, cot)
        _assert_fp32_inside_cap(tag, cell.ref(x, cot, dtype=torch.float32), g, F, div)
        return g
    ref_g = _cached(key, ref)
    got = cell.vjp(x, cot)
    _check_outliers(tag, got, ref_g, F, div)
    return x, cot, got


@FORMS
@pytest.mark.parametrize("name", ["A1", "A2", "A2c"])
def test_a_dense(dev, mode, cell_form, name):
    """A dense cotangent on every frame (masked ones included), the last sequence fully valid: every split and
    every column-reduction split adds its share.  Too many activations for the margin: the outlier form per slice."""
    (B, T, F, r, K), _ = A_SHAPES[name]
    _assert_a_plan(name)
    cell = Cell(dev, B, T, F, r, K, untied=("log_D", "log_alph", "log_lam1"), seed=_seed("A", name))
    _dense_outlier_case(cell, "A %s %s/%s dense" % (mode, name, cell_form), ("Ad", name))


# F = 34: two tail bins, M = Fp = 48, the permuted rows of EpiP1 / EpiP2 stop at 32; F = 21: no tail; the d log_D map
# with 17 groups (F = 65: a second round of 16 in dlogd_apply_kernel), 6 (F = 21: one clamped round) and, F = 2040,
# 128 groups of 16 bins (bpt = 4: 8 rounds)
A5_CASES = {34: ("vec", 1, 9), 21: ("vec", 1, 6), 65: ("vec", 1, 17), 2040: ("vec", 4, 128)}


@FORMS
@pytest.mark.parametrize("F", sorted(A5_CASES))
def test_a_bin_edges_and_dlogd_forms(dev, mode, cell_form, F):
    B, T, r, K = (2, 3, 6, 2) if F == 2040 else (3, 6, 6, 2)
    assert R.dlogd_form(F, 2 * r) == A5_CASES[F]
    assert (R.ntail_of(F), R.bptt_gemm_m(F), 16 * R.nft_main_of(F)) == \
        {34: (2, 48, 32), 21: (0, 32, 32), 65: (1, 64, 64), 2040: (0, 2048, 2048)}[F]
    cell = Cell(dev, B, T, F, r, K, untied=("log_D", "log_alph", "log_lam1"), seed=_seed("A5", F))
    x, cot = _dense_input(cell, np.random.default_rng(F))
    tag = "A %s F%d/%s" % (mode, F, cell_form)

    def ref():
        _assert_margin(tag, cell.margin(x))
        return cell.ref(x, cot)
    _check_max(tag + " dense", cell.vjp(x, cot), _cached(("A5", F), ref), F)
    fail = []
    _one_frame(cell, tag + " one-frame-last", B - 1, T - 1, fail, ("A5f", F))
    assert not fail, "\n".join(fail)


def _poison_next_allocations(cell, dev, poison):
    """Fresh memory for the next vjp that held `poison`: the forward workspace is dropped and torch's cache emptied,
    then whole segments of torch's allocator are filled with the pattern and freed -- 20 MiB ones (what it carves
    allocations of 1 .. 10 MiB from), 2 MiB ones (those below 1 MiB) and 256 MiB for anything larger: it hands a
    cached block out before it asks the driver for new memory.  Whether the block it gives for the BPTT workspace
    holds the pattern is printed.  Returns that workspace's size."""
    import ctypes
    from drnmf_amd import _capi
    desc = cell.model.cell._train_ctx[0]
    need_b = _capi.lib().drnmf_cell_backward_workspace_bytes(ctypes.byref(desc))
    cell.model.cell._ws.clear()
    torch.cuda.empty_cache()
    sizes = [20 << 18] * 6 + [(1 << 18) - 128] * 8 + [64 << 20]
    held = [torch.full((n,), poison, dtype=torch.float32, device=dev) for n in sizes]
    del held                                              # ... stays in torch's cache: the next allocations
    probe = torch.empty(need_b, dtype=torch.uint8, device=dev)[:need_b // 4 * 4].view(torch.float32)
    ok = bool(torch.isnan(probe).all()) if poison != poison else bool((probe == poison).all())
    del probe
    # (printed, not asserted: which block torch hands out depends on what else the process holds)
    print("EDGE A - poison-%r bwd-workspace-from-poisoned-memory %d" % (poison, ok))
    return need_b


@FORMS
def test_a_poisoned_memory(dev, mode, cell_form):
    """A1 dense on fresh allocations that held NaN and 1e30 (forward workspace, hiddens, BPTT workspace, outputs):
    bitwise the clean run -- the empty split 7 stores its zeros, nothing reads what it did not write."""
    (B, T, F, r, K), _ = A_SHAPES["A1"]
    assert _assert_a_plan("A1")[1] == [7]
    cell = Cell(dev, B, T, F, r, K, untied=("log_D", "log_alph", "log_lam1"), seed=_seed("A", "A1"))
    x, cot = _dense_input(cell, np.random.default_rng(7))
    clean = cell.vjp(x, cot)
    assert all(np.isfinite(clean[a]).all() for a in ARRAYS)
    for poison in (float("nan"), 1e30):
        _poison_next_allocations(cell, dev, poison)
        got = cell.vjp(x, cot)
        for a in ARRAYS:
            assert np.array_equal(got[a], clean[a]), "A %s A1/%s poison %r changed %s" % (mode, cell_form, poison, a)


@pytest.mark.parametrize("divergence,beta", [("kl", 1.5), ("beta", 1.5)])
def test_a_kl_beta(dev, mode, divergence, beta):
    """A2 on the KL / beta cell (unpack_g_kernel, state_matrix_kernel, the K0 instance of bwd_a_kernel, M = Fp and no
    odd-bin row): dense and one-frame first / last row.  (That cell has the factored form only.)"""
    (B, T, F, r, K), _ = A_SHAPES["A2"]
    assert R.tn_plan(R.bptt_gemm_m(F, divergence), 2 * r, B * T) == (2, []) and not R.odd_bin(F, divergence)
    cell = Cell(dev, B, T, F, r, K, untied=("log_D", "log_alph", "log_lam1"), seed=_seed("A8", divergence),
                divergence=divergence, beta=beta)
    tag = "A %s A2-%s" % (mode, divergence)
    _dense_outlier_case(cell, tag + " dense", ("A8d", divergence))
    fail = []
    for pname, bt in (("first", 0), ("last", B * T - 1)):
        _one_frame(cell, "%s one-frame-%s(bt=%d)" % (tag, pname, bt), bt // T, bt % T, fail, ("A8f", divergence))
    assert not fail, "\n".join(fail)


# ---- B: the loss heads alone (both modes) ----------------------------------------------------------------------

HEAD_R = (1, 3, 4, 6, 17)
HEAD_F = (5, 16, 21, 33, 257)
HEAD_ROWS = (1, 4, 5, 1023, 1025, 1540)


def _head_problem(rows, F, r, wide, square, seed, one_row=None):
    """hidden >= 0 and sparse, one all-zero row, one row zero in the clean half; x, y, weights 0 / 0.5 / 1 / 1.7 (or
    one live row); mask, A, Bn from the fp64 head rounded to fp32; wide: hidden is the last of K = 3 blocks of a
    [rows, 3 * 2r] tensor whose other columns hold 1e30."""
    rng = np.random.default_rng(seed)
    hid = (rng.random((rows, 2 * r)) * (rng.random((rows, 2 * r)) < 0.5)).astype(np.float32)
    zero_row = clean_zero = None
    if rows >= 4:
        zero_row, clean_zero = rows // 2, rows - 1
        hid[zero_row] = 0.0
        hid[clean_zero, :r] = 0.0
        hid[clean_zero, r:] += 0.1
    x = rng.random((rows, F)).astype(np.float32)
    y = rng.random((rows, F)).astype(np.float32)
    if one_row is None:
        w = rng.choice(np.array([0.0, 0.5, 1.0, 1.7], np.float32), size=rows)
        w[0] = 0.5
        if zero_row is not None:
            w[zero_row], w[clean_zero] = 1.0, 1.7
    else:
        w = np.zeros(rows, np.float32)
        w[one_row] = 1.7
    kc = (0.3 * rng.standard_normal((r, F))).astype(np.float32)
    kn = (0.3 * rng.standard_normal((r, F))).astype(np.float32)
    m, A, Bn = (a.astype(np.float32) for a in R.head_forward_ref(hid, kc, kn, square))
    buf, h_off = hid, 0
    if wide:
        buf = np.full((rows, 3 * 2 * r), 1e30, np.float32)
        h_off = 2 * 2 * r
        buf[:, h_off:] = hid
    return dict(hid=hid, buf=buf, h_off=h_off, x=x, y=y, w=w, kc=kc, kn=kn, m=m, A=A, Bn=Bn, zero_row=zero_row)


def _check_head(tag, sums, d_h, d_kc, d_kn, ref, zero_row, fail):
    s = sums.cpu().numpy().astype(np.float64)
    lerr = abs(s[0] - ref[0]) / max(abs(ref[0]), 1e-30)
    got = {"d_hidden": d_h.cpu().numpy().astype(np.float64), "d_kc": d_kc.cpu().numpy().astype(np.float64),
           "d_kn": d_kn.cpu().numpy().astype(np.float64)}
    want = dict(zip(("d_hidden", "d_kc", "d_kn"), ref[2:]))
    errs = [(n, _rel(got[n], want[n])) for n in ("d_hidden", "d_kc", "d_kn")]
    if zero_row is not None:
        # 1e-7 + A + Bn = 1e-7 on the all-zero row: its d hidden is 1e7 times the others' and would hide them
        rest = np.arange(got["d_hidden"].shape[0]) != zero_row
        errs += [("d_hidden[zero-row]", _rel(got["d_hidden"][zero_row], want["d_hidden"][zero_row])),
                 ("d_hidden[other-rows]", _rel(got["d_hidden"][rest], want["d_hidden"][rest]))]
    print("EDGE %s loss %.3e" % (tag, lerr))
    for n, e in errs:
        print("EDGE %s %s %.3e" % (tag, n, e))
    if s[1] != ref[1]:
        fail.append("%s: count %r, reference %r" % (tag, s[1], ref[1]))
    if not lerr <= L_TOL:
        fail.append("%s: loss %r, reference %r" % (tag, s[0], ref[0]))
    fail += ["%s %s: max|d|/max|ref| = %.3e" % (tag, n, e) for n, e in errs if not e <= G_TOL]


def _run_head(dev, p, square, l1=None):
    from drnmf_amd import ops
    d = lambda a: _dv(a, dev)
    if l1 is None:
        return ops.loss_head_backward(d(p["x"]), d(p["buf"]), d(p["kc"]), d(p["kn"]), d(p["m"]), d(p["A"]),
                                      d(p["Bn"]), d(p["y"]), d(p["w"]), square=square, h_off=p["h_off"])
    return ops.snmf_cost_head_backward(d(p["x"]), d(p["buf"]), d(p["kc"]), d(p["kn"]), d(p["A"]), d(p["Bn"]),
                                       d(p["w"]), l1, h_off=p["h_off"])


@pytest.mark.parametrize("rows", HEAD_ROWS)
def test_b_loss_head_alone(dev, mode, rows):
    """drnmf_loss_head_backward at every r x F of the tables (r % 4 and the Fp4 padding present and absent), the
    layout (h_off, ld_h) = (0, 2r) / (2 * 2r, 3 * 2r) and `square` alternating so that every r and every F meets
    both; rows across the 4-row blocks (1, 4, 5), the 256 partials of final_sums_kernel (1023 -> 256 blocks, 1025 ->
    257) and the split-K of the kernel gradient (1540: 8 splits, the last one empty)."""
    assert R.head_plan(1540, 33, 6) == (36, 385, 8, [7]) and R.head_plan(1023, 33, 6)[1:3] == (256, 5)
    assert R.head_plan(1025, 33, 6)[1:3] == (257, 5) and R.head_plan(5, 33, 6)[1:] == (2, 1, [])
    fail = []
    for ri, r in enumerate(HEAD_R):
        for fi, F in enumerate(HEAD_F):
            wide, square = bool((ri + fi) % 2), bool((ri + fi // 2 + fi) % 2)
            p = _head_problem(rows, F, r, wide, square, seed=10000 * rows + 100 * r + F)
            ref = _cached(("B", rows, r, F), lambda: R.head_loss_and_grads(p["x"], p["hid"], p["kc"], p["kn"], p["y"],
                                                                            p["w"], square))
            sums, d_h, d_kc, d_kn = _run_head(dev, p, square)
            torch.cuda.synchronize()
            tag = "B %s rows%d-r%d-F%d-%s%s" % (mode, rows, r, F, "wide" if wide else "own", "-square" if square else "")
            _check_head(tag, sums, d_h, d_kc, d_kn, ref, p["zero_row"], fail)
    assert not fail, "\n".join(fail)


def test_b_loss_head_weight_on_one_row(dev, mode):
    """w non-zero on ONE of 1540 rows, at the positions of A1: the kernel gradients are that row's outer product --
    of split 0, of the partial k-tile in front of the empty split, of either side of a split boundary."""
    rows, F, r = 1540, 33, 6
    assert R.head_plan(rows, F, r) == (36, 385, 8, [7])
    fail = []
    for pname, row in sorted(_positions(7, 220, 8).items(), key=lambda kv: kv[1]):
        for square in (False, True):
            p = _head_problem(rows, F, r, True, square, seed=row, one_row=row)
            p["hid"][row] += 0.05                         # (the live row has every atom active)
            p["buf"][:, p["h_off"]:] = p["hid"]
            p["m"], p["A"], p["Bn"] = (a.astype(np.float32) for a in
                                       R.head_forward_ref(p["hid"], p["kc"], p["kn"], square))
            ref = _cached(("B1", row, square), lambda: R.head_loss_and_grads(p["x"], p["hid"], p["kc"], p["kn"],
                                                                             p["y"], p["w"], square))
            assert ref[1] == 1.0 and np.abs(ref[3]).max() > 0 and np.abs(ref[4]).max() > 0
            sums, d_h, d_kc, d_kn = _run_head(dev, p, square)
            torch.cuda.synchronize()
            tag = "B %s one-row-%s(row=%d)%s" % (mode, pname, row, "-square" if square else "")
            _check_head(tag, sums, d_h, d_kc, d_kn, ref, None, fail)
    assert not fail, "\n".join(fail)


@pytest.mark.parametrize("rows", [5, 1540])
def test_b_snmf_cost_head_alone(dev, mode, rows):
    """drnmf_snmf_cost_head_backward: r in {3, 6}, F in {21, 33}, both layouts."""
    fail = []
    for r in (3, 6):
        for F in (21, 33):
            for wide in (False, True):
                p = _head_problem(rows, F, r, wide, False, seed=rows + 10 * r + F)
                l1 = 0.3 * 2 * r / F
                ref = _cached(("Bs", rows, r, F), lambda: R.snmf_cost_head_grads(p["x"], p["hid"], p["kc"], p["kn"],
                                                                                  p["w"], l1))
                sums, d_h, d_kc, d_kn = _run_head(dev, p, False, l1)
                torch.cuda.synchronize()
                tag = "B %s snmf-cost-rows%d-r%d-F%d-%s" % (mode, rows, r, F, "wide" if wide else "own")
                _check_head(tag, sums, d_h, d_kc, d_kn, ref, None, fail)
    assert not fail, "\n".join(fail)


# ---- C: the BPTT alone on cotangents of the test's choosing (both forms) ---------------------------------------

C_SHAPE = (5, 9, 33, 8)
C_VARIANTS = {
    "untied": dict(K=3, untied=("log_D", "log_alph")),
    "untie_alph": dict(K=3, untied=("log_D", "log_alph"), untie_alph=True),
    "tied": dict(K=3, untied=()),
    "K1": dict(K=1, untied=("log_D", "log_alph")),
}


def _c_input(x0, mask_value=-1.0):
    """Row 0: valid, then masked to the end; row 1: masked frames 0 .. 2 first; row 2: fully masked; row 3: masked
    frames 3, 4 in the middle; row 4: fully valid."""
    x = x0.copy()
    x = _fill_row(_fill_row(_fill_row(x, 1), 3), 4)
    x[0, 6:] = -1.0
    x[1, :3] = -1.0
    x[2] = -1.0
    x[3, 3:5] = -1.0
    if mask_value != -1.0:
        x[x == -1.0] = mask_value
    valid = (x != mask_value).any(-1)
    seen = np.cumsum(valid, axis=1) > 0
    assert valid[0, :6].all() and not valid[0, 6:].any() and not valid[2].any() and valid[4].all()
    return x, valid, seen


def _c_cotangents(cell, x, valid, seen, rng):
    B, T = valid.shape
    dense = rng.standard_normal((B, T, cell.N)).astype(np.float32)
    after = dense * (~valid & seen)[..., None]           # masked frames behind a valid one: handed to that frame
    before = dense * (~seen)[..., None]                  # nothing valid yet (row 1's head, all of row 2): no gradient
    interior = np.zeros_like(dense)
    interior[3, 3:5] = dense[3, 3:5]
    h = cell.hidden(x)
    impulse = np.zeros_like(dense)
    impulse[4, 5, int(np.argmax(h[4, 5]))] = 1.0
    assert h[4, 5].max() > 0 and after.any() and before.any()
    return dict(dense=dense, masked_after_valid=after, interior_masked=interior, impulse=impulse), before


@FORMS
@pytest.mark.parametrize("variant", sorted(C_VARIANTS))
def test_c_bptt_alone(dev, cell_form, variant):
    B, T, F, r = C_SHAPE
    v = C_VARIANTS[variant]
    cell = Cell(dev, B, T, F, r, seed=_seed("C", variant), **v)
    x, valid, seen = _c_input(cell.x0)
    tag = "C f32 %s/%s" % (variant, cell_form)
    cots, before = _c_cotangents(cell, x, valid, seen, np.random.default_rng(3))

    def refs():
        _assert_margin(tag, cell.margin(x))
        return {n: cell.ref(x, c) for n, c in cots.items()}
    ref = _cached(("C", variant), refs)
    fail = []
    for n, c in sorted(cots.items()):
        assert np.abs(ref[n]["d_log_D"]).max() > 0, n
        _check_max("%s %s" % (tag, n), cell.vjp(x, c), ref[n], F, _slices if n == "dense" else _whole, fail=fail)
    assert not fail, "\n".join(fail)
    _assert_zero(tag + " before-first-valid", cell.vjp(x, before))


@FORMS
def test_c_bptt_alone_with_an_entering_state(dev, cell_form):
    """The entering state is a constant of the gradient: d log_h0 exactly 0, everything else against cell_vjp."""
    B, T, F, r = C_SHAPE
    cell = Cell(dev, B, T, F, r, seed=_seed("C", "state"), **C_VARIANTS["untied"])
    x, valid, seen = _c_input(cell.x0)
    state = (0.2 * np.random.default_rng(9).random((B, cell.N))).astype(np.float32)
    tag = "C f32 state/%s" % cell_form
    cots, before = _c_cotangents(cell, x, valid, seen, np.random.default_rng(4))

    def refs():
        _assert_margin(tag, cell.margin(x, state=state))
        return {n: cell.ref(x, cots[n], state=state) for n in ("dense", "masked_after_valid")}
    ref = _cached(("Cs",), refs)
    for n in ("dense", "masked_after_valid"):
        got = cell.vjp(x, cots[n], state=state)
        assert not ref[n]["d_log_h0"].any() and not got["d_log_h0"].any(), "%s %s: d_log_h0 must be exactly 0" % (tag, n)
        _check_max("%s %s" % (tag, n), got, ref[n], F, _slices if n == "dense" else _whole)
    _assert_zero(tag + " before-first-valid", cell.vjp(x, before, state=state))


@pytest.mark.parametrize("divergence", ["kl", "beta"])
def test_c_bptt_alone_kl_beta(dev, divergence):
    B, T, F, r = C_SHAPE
    cell = Cell(dev, B, T, F, r, seed=_seed("C", divergence), divergence=divergence, **C_VARIANTS["untied"])
    x, valid, seen = _c_input(cell.x0)
    tag = "C f32 %s" % divergence
    cots, before = _c_cotangents(cell, x, valid, seen, np.random.default_rng(5))

    def refs():
        _assert_margin(tag, cell.margin(x))
        return {n: cell.ref(x, cots[n]) for n in ("dense", "masked_after_valid")}
    ref = _cached(("Ck", divergence), refs)
    for n in ("dense", "masked_after_valid"):
        _check_max("%s %s" % (tag, n), cell.vjp(x, cots[n]), ref[n], F, _slices if n == "dense" else _whole, divergence)
    _assert_zero(tag + " before-first-valid", cell.vjp(x, before))


# ---- D: graph chunks -------------------------------------------------------------------------------------------

def _same(tag, a, b):
    for n in ARRAYS:
        assert np.array_equal(a[n], b[n]), "%s: %s differs" % (tag, n)


@pytest.mark.parametrize("K,T", [(7, 1), (7, 60), (7, 61), (7, 62), (7, 122), (7, 123), (2, 64), (2, 65)],
                         ids=lambda v: str(v))
def test_d_graph_chunks(dev, monkeypatch, K, T):
    """The factored chain in graphs of frames_per_graph(K, T) frames plus single-frame graphs for the rest: K = 7
    -> 13 launches a frame, 61 frames a graph; K = 2 -> 64.  Against cell_vjp, a second time (the cached graphs
    replayed: bitwise), and as direct launches (DRNMF_NO_GRAPH=1: the same kernels on the same arguments in the
    same order, so bitwise again)."""
    monkeypatch.setenv("DRNMF_GRAM", "0")
    B, F, r = 3, 21, 6
    assert R.frames_per_graph(K, T) == {(7, 1): 1, (7, 60): 60, (7, 61): 61, (7, 62): 61, (7, 122): 61, (7, 123): 61,
                                        (2, 64): 64, (2, 65): 64}[(K, T)]
    assert not R.gram_of(B, 2 * r, K, env=0)
    cell = Cell(dev, B, T, F, r, K, seed=_seed("D", K, T))
    x, cot = _dense_input(cell, np.random.default_rng(T))
    tag = "D f32 K%dT%d" % (K, T)

    def ref():
        g = cell.ref(x, cot)
        if T == 1:
            _assert_margin(tag, cell.margin(x))
        else:
            _assert_fp32_inside_cap(tag, cell.ref(x, cot, dtype=torch.float32), g, F)
        return g
    ref_g = _cached(("D", K, T), ref)
    g1 = cell.vjp(x, cot)
    if T == 1:
        _check_max(tag, g1, ref_g, F)
    else:
        _check_outliers(tag, g1, ref_g, F)
    _same(tag + " second replay", g1, cell.vjp(x, cot))
    monkeypatch.setenv("DRNMF_NO_GRAPH", "1")
    g3 = cell.vjp(x, cot)
    monkeypatch.delenv("DRNMF_NO_GRAPH")
    _same(tag + " direct launches against the graphs", g1, g3)


# ---- E: one dimension at a time across the tiles ---------------------------------------------------------------

E_BASE = dict(B=3, T=4, F=33, r=8, K=3)


def _vary(**kw):
    d = dict(E_BASE)
    d.update(kw)
    return tuple(d[c] for c in ("B", "T", "F", "r", "K"))


E_SHAPES = [_vary(B=B) for B in (1, 15, 16, 17, 33)] + [_vary(r=r) for r in (1, 15, 16, 17, 31, 32, 33)] + \
    [_vary(F=F) for F in (15, 16, 17, 18, 19, 31, 32, 35, 47, 48, 49)] + [_vary(T=1), _vary(T=2, K=5)]
_eid = lambda s: "B%dT%dF%dr%dK%d" % s


def _dense_max_case(dev, tag, shape, key, seed, **kw):
    B, T, F, r, K = shape
    cell = Cell(dev, B, T, F, r, K, untied=("log_D", "log_alph", "log_lam1"), seed=seed, **kw)
    x, cot = _dense_input(cell, np.random.default_rng(sum(shape)))

    def ref():
        _assert_margin(tag, cell.margin(x))
        return cell.ref(x, cot)
    _check_max(tag, cell.vjp(x, cot), _cached(key, ref), F)
    return cell


@FORMS
@pytest.mark.parametrize("shape", E_SHAPES, ids=_eid)
def test_e_tile_edges(dev, cell_form, shape):
    """B across the 16-row tiles, N = 2 r across the 32-atom blocks and 16-atom tiles, F across the 16-bin tiles with
    0, 1, 2 tail bins and 3 (no tail path), T = 1, K > T: dense cotangent, per-slice bound."""
    _dense_max_case(dev, "E f32 %s/%s" % (_eid(shape), cell_form), shape, ("E", shape), _seed("E", shape))


# (B, r, DRNMF_RB, DRNMF_KS) -> (RB, KS, chunks per range) by hand
E_TUNED = {
    (1, 8, 2, None): (2, 1, 2), (17, 8, 2, None): (2, 1, 2), (33, 8, 2, None): (2, 1, 2),
    (3, 65, None, None): (1, 2, 5),          # Np = 160: 10 chunks
    (3, 130, None, None): (1, 4, 5),         # Np = 288: 18 chunks in ranges of 5, 5, 5, 3
    (3, 170, None, 8): (1, 8, 3),            # Np = 352: 22 chunks in ranges of 3 x 7, 1 -- the rule never chooses 8
    (3, 130, None, 8): (1, 4, 5),            # 18 chunks in 8 ranges of 3 would leave two empty: not taken
}


@FACTORED
@pytest.mark.parametrize("case", sorted(E_TUNED, key=str), ids=lambda c: "B%d-r%d-RB%s-KS%s" % c)
def test_e_row_blocks_and_atom_ranges(dev, cell_form, monkeypatch, case):
    """The row-blocked kernels (DRNMF_RB=2; B = 1: the second row block is all padding) and the atom-range instances
    KS = 2, 4 (uneven ranges) and 8 of cell_b / bwd_a, through the library's own tuning variables."""
    B, r, rb, ks = case
    shape = _vary(B=B, r=r)
    F = shape[2]
    if rb is not None:
        monkeypatch.setenv("DRNMF_RB", str(rb))
    if ks is not None:
        monkeypatch.setenv("DRNMF_KS", str(ks))
    assert (R.rb_of(B, F, 2 * r, rb),) + R.ks_of(B, F, 2 * r, ks, rb) == E_TUNED[case]
    _dense_max_case(dev, "E f32 %s-RB%s-KS%s" % (_eid(shape), rb, ks), shape, ("E", shape), _seed("E", shape))


def test_e_qred(dev, monkeypatch):
    """N = 2080: 65 atom blocks > 64 and one tail bin -- the backward's cell_b adds the odd-bin partials (dqsum) and
    bwd_a_kernel<G, KS, true> reads the sums.  37 k activations: the outlier form per slice, and the last row alone
    under the plain bound."""
    monkeypatch.setenv("DRNMF_GRAM", "0")
    B, T, F, r, K = 3, 3, 257, 1040, 2
    assert R.qred_of(B, F, 2 * r) and R.ks_of(B, F, 2 * r) == (4, 33) and R.ntail_of(F) == 1
    assert not R.qred_of(B, F, 2000) and not R.gram_of(B, 2 * r, K, env=0)
    cell = Cell(dev, B, T, F, r, K, seed=_seed("E", "qred"))
    _dense_outlier_case(cell, "E f32 qred dense", ("Eq",))
    fail = []
    _one_frame(cell, "E f32 qred one-frame-last", B - 1, T - 1, fail, ("Eqf",))
    assert not fail, "\n".join(fail)


@FORMS
@pytest.mark.parametrize("N", [7, 33])
def test_e_odd_n_through_ops(dev, cell_form, N):
    """A descriptor the model never builds (N = 2 r there): odd N through ops.cell_forward / ops.cell_backward.
    validate_cell_desc admits it (include/drnmf.h documents no restriction); bwd_edge_kernel takes its element-wise
    path (pair == false), the scalar gemm_tn, colreduce<1,1,8> and dlogd_kernel.  U1 = 0.9 I + 0.02, Uk = 0.01: every
    U term of the state gradient is live."""
    from drnmf_amd import ops
    B, T, F, K = 3, 4, 33, 3
    assert R.colreduce_form(N) == (1, 1, 8) and R.dlogd_form(F, N) == ("scalar", 0, 0)
    rng = np.random.default_rng(_seed("E", "oddN", N))
    W = rng.random((F, N)) ** 2 + 0.01
    log_D = np.stack([np.log(W) + 0.05 * rng.standard_normal((F, N)) for _ in range(K)]).astype(np.float32)
    log_alph = np.log(N / 4.0 + 0.5 * rng.random((K, 1))).astype(np.float32)
    log_lam1 = np.log(np.array([0.1], np.float32))
    log_h0 = rng.uniform(-0.05, 0.05, N).astype(np.float32)
    u = (0.92, 0.02, 0.01)
    x = (rng.random((B, T, F)) * (rng.random((B, T, F)) < 0.6)).astype(np.float32) + 0.01
    x[1, 0] = -1.0
    x[2, 2:] = -1.0
    cot = rng.standard_normal((B, T, N)).astype(np.float32)
    alt = {"log_U1": np.log(np.where(np.eye(N, dtype=bool), u[0], u[1])), "log_Uk": np.log(np.full((N, N), u[2])),
           "log_lam1": log_lam1[0].astype(np.float64)}
    labels = {"log_D": ["log_D_%d" % k for k in range(K)], "log_alph": ["log_alph_%d" % k for k in range(K)],
              "log_lam1": ["log_lam1"] * K}
    for k in range(K):
        alt["log_D_%d" % k], alt["log_alph_%d" % k] = log_D[k], log_alph[k, 0]
    tag = "E f32 odd-N%d/%s" % (N, cell_form)

    def ref():
        _assert_margin(tag, R.relu_margin(x, alt, labels, K, log_h0))
        return _stack(R.cell_vjp(x, alt, labels, K, log_h0, cot), labels)
    ref_g = _cached(("Eo", N), ref)
    desc = ops.make_desc(B, T, F, N, K, n_D=K, n_alph=K, alph_len=1, n_lam=1, return_all_hidden=True)
    params = ops.prepare_params(desc, _dv(log_D, dev), _dv(log_alph, dev), _dv(log_lam1, dev))
    ws = ops.cell_workspace(desc, dev)
    xd, lh = _dv(x, dev), _dv(log_h0, dev)
    hall = ops.cell_forward(xd, -1.0, params, desc, lh, u, workspace=ws)
    g = ops.cell_backward(xd, params, desc, lh, u, hall, _dv(cot, dev), ws)
    torch.cuda.synchronize()
    _check_max(tag, {k: g[k].cpu().numpy().astype(np.float64) for k in ARRAYS}, ref_g, F)


# ---- F: mask_value 0.0 -----------------------------------------------------------------------------------------

@FORMS
def test_f_mask_value_zero(dev, cell_form):
    """mask_value = 0.0: a frame of real zeros is a masked frame (and single zero bins are input).  The C input with
    its masked frames as zeros; forward and backward agree with the reference on which frames those are."""
    B, T, F, r = C_SHAPE
    cell = Cell(dev, B, T, F, r, seed=_seed("F", 0.0), **C_VARIANTS["untied"])
    x, valid, seen = _c_input(cell.x0, mask_value=0.0)
    x[4, 2, 3] = x[1, 5, 0] = 0.0                         # zero bins of valid frames
    assert not (x == -1.0).any() and (x[valid] == 0.0).any() and valid[4, 2] and valid[1, 5] and (~valid).sum() == 3 + 3 + T + 2
    cot = np.random.default_rng(6).standard_normal((B, T, cell.N)).astype(np.float32)
    tag = "F f32 mask0/%s" % cell_form

    def ref():
        _assert_margin(tag, cell.margin(x, mask_value=0.0))
        h = cell.hidden(x, mask_value=0.0)
        assert np.array_equal(h[0, 6:], np.broadcast_to(h[0, 5], h[0, 6:].shape)) and not h[2].any()
        return cell.ref(x, cot, mask_value=0.0)
    _check_max(tag + " dense", cell.vjp(x, cot, mask_value=0.0), _cached(("F",), ref), F)
