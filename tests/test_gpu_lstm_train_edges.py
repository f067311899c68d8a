"""The LSTM baseline's training kernels (csrc/lstm.hip: stashing forward, loss head, BPTT wavefront, time-batched
weight gradients) at the shapes where they take another path, against the fp64 references of
tests/lstm_train_ref.py.  The forward has tests/test_gpu_lstm_edges.py; this is its counterpart for the gradients.

  A  split-K weight gradients (gemm_tn with 2 .. 32 splits, empty trailing splits, partial last k-tiles) and the
     bias column sums with 4 .. 32 splits: dense weights, weight on ONE sequence (so that a lost k-tile is the
     whole gradient, not 0.5 % of it), a NaN-filled workspace;
  B  the loss head alone on a hidden tensor of the test's choosing (ld_h == H scalar paths, padded rows, F and
     B T across the 4-wide groups and the 256 threads of the final reduction);
  C  the BPTT alone on a cotangent of the test's choosing (dense, on masked frames only, impulses, an entering
     state);
  D  lengths across the 64-frame graphs of the two training chains, replayed twice and against direct launches;
  E  one dimension at a time across the 32-unit / 16-row / 4-bin tiles, T = 1 and K > T;
  F  mask_value 0.0 and None.

Groups marked "both modes" run with the frame-parallel products in exact fp32 and in the split-operand mode.

Bounds: those of tests/test_gpu_lstm_train.py -- G_TOL on max|d| / max|ref| per array, L_TOL on the loss, the
count exact.  hard_sigmoid has kinks where an fp32 pre-activation can fall on the other side than the fp64 one
and the derivative jumps by 0.2; with a max-based bound that has to be excluded, so every hard_sigmoid case first
asserts lstm_train_ref.kink_margin >= KINK (computed from the fp64 reference alone: a condition on the INPUT, not
a tolerance), and its seed (SEEDS) was picked for that.  The long dense cases of A use sigmoid: a million
hard-sigmoid gates always have one next to a kink.  D's hard_sigmoid cases use weights of scale 0.5 (every gate
inside the linear range) for the same reason; what they test is the chunking.

Every check prints "EDGE <group> <mode> <case> <array> <error>" before it asserts.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import lstm_ref as R
import lstm_state_ref as SR
import lstm_train_ref as TR

pytestmark = pytest.mark.gpu

G_TOL = 2e-3
L_TOL = 1e-5
KINK = 1e-4
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


@contextlib.contextmanager
def _matrix_mode(name, dev):
    from drnmf_amd import ops
    prev = ops.set_matrix_mode(name, dev)
    try:
        yield name
    finally:
        ops.set_matrix_mode(prev, dev)


@pytest.fixture(params=["f32", "bf16x3"])
def mode(request, dev):
    """The handle's matrix mode for the test, the previous one restored afterwards."""
    with _matrix_mode(request.param, dev) as m:
        yield m


# ---- the split rules, restated -----------------------------------------------------------------------------------

def pick_splits(M, N, rows, max_splits=32):
    """gemm_tn::pick_splits (csrc/gemm_tn.h) as lstm_tn_product calls it, restated: this mirror CANNOT SEE THE
    HEADER.  It exists so that a case named after a split count fails its precondition when the rule it was
    computed with is no longer the one written here -- whoever changes the rule in the header changes it here and
    re-derives the cases."""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    best, best_cost = 1, 1e30
    for s in range(1, max_splits + 1):
        if s > 1 and rows // s < 192:
            break
        cost = ((tiles * s + 511) // 512) / s * (1.0 + 0.004 * s)
        if cost < best_cost - 1e-9:
            best, best_cost = s, cost
    return best


def empty_splits(rows, splits):
    """work_of: split s takes the k-tiles (32 rows each) [s per, (s + 1) per) with per = ceil(#k-tiles / splits);
    the splits whose range starts behind the last k-tile have nothing to add and must store zeros."""
    nkt = (rows + 31) // 32
    per = (nkt + splits - 1) // splits
    return [s for s in range(splits) if s * per >= nkt]


def colsum_splits(rows):
    """lstm_colsum: 32 splits, halved while a split would get fewer than 64 rows (the same caveat as pick_splits)."""
    s = 32
    while s > 1 and rows // s < 64:
        s >>= 1
    return s


def split_plan(B, T, F, H):
    """(splits of the BPTT products, of the head product, empty BPTT splits, empty head splits, colsum splits of
    the BPTT, of the head) -- every BPTT product of a model gets the same count here (asserted)."""
    Fq, Hq, NC = _rup(F, 4), _rup(H, 4), _rup(H, 8) * 4
    rb, rh = B * (T + 1), B * T
    sb = {pick_splits(Hq, NC, rb), pick_splits(Fq, NC, rb)}
    assert len(sb) == 1
    sb = sb.pop()
    sh = pick_splits(Hq, Fq, rh)
    return sb, sh, empty_splits(rb, sb), empty_splits(rh, sh), colsum_splits(rb), colsum_splits(rh)


# ---- problems and runs -------------------------------------------------------------------------------------------

# seeds of the hard_sigmoid cases, picked so that kink_margin >= KINK (each case asserts it)
SEEDS = {("A", (33, 194, 18, 13, 2), "first"): 1, ("A", (32, 200, 21, 37, 2), "first"): 2,
         ("A", (32, 200, 21, 37, 2), "straddle"): 5, ("E", (5, 6, 9, 16, 2)): 1, ("E", (15, 6, 9, 10, 2)): 1,
         ("F", 0.0): 1, ("F", None): 1}                       # (every other case: seed 0)


def _problem(shape, seed, scale=1.5, mask_value=-1.0, flip=False):
    """Input with every mask pattern, targets, temporal weights (a few valid frames without weight, a few masked
    ones with) and Keras weights, all from one seed.  flip: the sequences in reverse order, so that the LAST one
    is the fully valid one (otherwise the first)."""
    B, T, F, H, K = shape
    rng = np.random.default_rng(seed)
    x, valid = R.masked_input(rng, B, T, F, "mixed", -1.0 if mask_value is None else mask_value)
    if flip:
        x, valid = np.ascontiguousarray(x[::-1]), np.ascontiguousarray(valid[::-1])
    if mask_value is None:
        valid = np.ones_like(valid)
    y = rng.random((B, T, F)).astype(np.float32)
    w = valid.astype(np.float32)
    w[rng.random((B, T)) < 0.1] = 0.0
    w[rng.random((B, T)) < 0.05] = 0.5
    if not valid.all():                                      # a masked frame with weight, whatever the draw
        w[tuple(np.argwhere(~valid)[0])] = 0.5
    if not w.any():
        w[0, 0] = 1.0
    wt = R.random_weights(rng, F, H, K, scale=scale)
    return x, valid, y, w, wt


def _model(dev, wt, K, act, mask_value=-1.0):
    from drnmf_amd import layers
    F, H = wt[0].shape[0], wt[1].shape[0]
    m = layers.build_lstm(dict(mask_value=mask_value, maxseq=8, input_dim=F, output_dim=F, K_layers=K,
                               hidden_dim=H, recurrent_activation=act), device=dev)
    m.set_weights(wt)
    m.compile()
    return m


def _dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _grads(m, dev, x, y, w):
    flat = m.loss_and_grads(_dv(x, dev), _dv(y, dev), _dv(w, dev))
    torch.cuda.synchronize()
    f = flat.cpu().numpy()
    return float(f[-4]), float(f[-3]), [m._gview[n].cpu().numpy() for n, _ in m._train_items]


_REFS = {}


def _cached(key, fn):
    """One fp64 reference per case, shared by the matrix modes (and never modified)."""
    if key not in _REFS:
        _REFS[key] = fn()
    return _REFS[key]


def _rel(got, ref):
    return float(np.max(np.abs(got - ref))) / max(float(np.max(np.abs(ref))), 1e-30)


def _names(K):
    return [n % k for k in range(K) for n in ("kernel_%d", "recurrent_%d", "bias_%d")] + ["w_out", "b_out"]


def _check(tag, got, ref, names, tol=G_TOL):
    """max|d| / max|ref| per array: all printed, then all asserted."""
    errs = [_rel(np.asarray(g, dtype=np.float64), r) for g, r in zip(got, ref)]
    assert len(errs) == len(names)
    for n, e in zip(names, errs):
        print("EDGE %s %s %.3e" % (tag, n, e))
    for n, e in zip(names, errs):
        assert e <= tol, "%s %s: max|d|/max|ref| = %.3e" % (tag, n, e)


def _check_loss(tag, sse, cnt, sse_r, cnt_r):
    err = abs(sse - sse_r) / max(abs(sse_r), 1e-30)
    print("EDGE %s loss %.3e" % (tag, err))
    assert cnt == cnt_r, "%s: count %r, reference %r" % (tag, cnt, cnt_r)
    assert err <= L_TOL, "%s: loss %r, reference %r" % (tag, sse, sse_r)


def _assert_margin(tag, x, wt, K, mask_value=-1.0, state=None):
    m = TR.kink_margin(x, wt, K, mask_value, state)
    assert m >= KINK, "%s: precondition -- a hard_sigmoid gate of the fp64 run lies %.2e from a kink" % (tag, m)


def _full_case(dev, tag, shape, act, seed, scale=1.5, mask_value=-1.0, test_loss=False, flip=False):
    """Model gradients and loss against fp64 autograd.  Returns (model, problem, gradients, reference gradients)."""
    K = shape[4]
    x, valid, y, w, wt = _problem(shape, seed, scale, mask_value, flip)

    def ref():
        if act == "hard_sigmoid":
            _assert_margin(tag, x, wt, K, mask_value)
        return TR.loss_and_grads(x, y, w, wt, K, mask_value, act)
    sse_r, cnt_r, gr = _cached((shape, act, seed, scale, mask_value, flip), ref)
    m = _model(dev, wt, K, act, mask_value)
    sse, cnt, gs = _grads(m, dev, x, y, w)
    _check_loss(tag, sse, cnt, sse_r, cnt_r)
    _check(tag, gs, gr, _names(K))
    if test_loss:
        got = float(m.test_on_batch(x, y, w))
        err = abs(got - sse_r / cnt_r) / abs(sse_r / cnt_r)
        print("EDGE %s test_on_batch %.3e" % (tag, err))
        assert err <= L_TOL, "%s: test_on_batch %r, reference %r" % (tag, got, sse_r / cnt_r)
    return m, (x, valid, y, w, wt), gs, gr


# ---- A: split-K weight gradients and column sums (both modes) ----------------------------------------------------

# (B, T, F, H, K) -> (BPTT splits, head splits, empty BPTT splits, empty head splits, colsum splits BPTT, head)
SPLIT_CASES = {
    (5, 77, 18, 13, 2): (2, 2, [], [], 4, 4),
    (16, 24, 21, 37, 2): (2, 2, [], [], 4, 4),
    (19, 40, 18, 37, 2): (4, 3, [], [], 8, 8),
    (20, 101, 21, 13, 2): (10, 10, [], [], 16, 16),
    (33, 194, 18, 13, 2): (32, 32, [29, 30, 31], [29, 30, 31], 32, 32),
    (32, 200, 21, 37, 2): (32, 32, [29, 30, 31], [29, 30, 31], 32, 32),
}
LONG = [(33, 194, 18, 13, 2), (32, 200, 21, 37, 2)]
_sid = lambda s: "B%dT%dF%dH%dK%d" % s


def _assert_plan(shape, want):
    B, T, F, H, _ = shape
    plan = split_plan(B, T, F, H)
    assert plan == want, "precondition: %s was chosen for the split plan %r, the rules now give %r" % (
        _sid(shape), want, plan)


@pytest.mark.parametrize("shape", sorted(SPLIT_CASES), ids=_sid)
def test_split_k_dense(dev, mode, shape):
    """Weight on (almost) every valid frame, sigmoid gates: every split adds its share, the last k-tile is partial
    (rows % 32 != 0 in all but (32, 200), where the rows end on a k-tile exactly).  The sequences are flipped: the
    last one, whose frames fill the tail k-tile, is fully valid (unflipped, (20, 101) would end on an all-masked
    sequence and its tail k-tile on zeros)."""
    _assert_plan(shape, SPLIT_CASES[shape])
    _full_case(dev, "A %s dense-%s" % (mode, _sid(shape)), shape, "sigmoid", seed=sum(shape), flip=True)


def test_split_k_production_width(dev, mode):
    """F = 513, H = 250: 5 x 8 output tiles of 128 x 128 per product, two splits; the max-based bound and, as the
    big case of test_gpu_lstm_train.py, the norm-based one."""
    shape = (4, 100, 513, 250, 2)
    _assert_plan(shape, (2, 2, [], [], 4, 4))
    tag = "A %s dense-%s" % (mode, _sid(shape))
    _, _, gs, gr = _full_case(dev, tag, shape, "sigmoid", seed=513, flip=True)
    for g, r, n in zip(gs, gr, _names(2)):
        rel = float(np.linalg.norm(g - r)) / max(float(np.linalg.norm(r)), 1e-30)
        print("EDGE %s-norm %s %.3e" % (tag, n, rel))
        assert rel <= G_TOL, "%s: |d|/|ref| = %.3e" % (n, rel)


def _straddler(B, T, valid):
    """The first sequence whose rows cross a boundary between two splits of 7 k-tiles = 224 rows, in the BPTT
    products (T + 1 rows per sequence) AND in the head product (T rows), with its last frame valid."""
    for b in range(1, B - 1):
        lo1, hi1 = b * (T + 1), (b + 1) * (T + 1) - 1
        lo0, hi0 = b * T, (b + 1) * T - 1
        if lo1 // 224 != hi1 // 224 and lo0 // 224 != hi0 // 224 and valid[b, -1]:
            return b
    raise AssertionError("no sequence straddles a split boundary")


@pytest.mark.parametrize("which", ["first", "last", "straddle"])
@pytest.mark.parametrize("shape", LONG, ids=_sid)
def test_split_k_weight_on_one_sequence(dev, mode, shape, which):
    """sample_weight nonzero on the last three frames of ONE sequence: every other row of the contraction adds an
    exact zero, so the gradient is the sum of a few k-tiles -- of split 0 (first), of the tail tile in front of
    the empty splits (last), of two neighbouring splits (straddle) -- and the reference is that sequence alone."""
    _assert_plan(shape, SPLIT_CASES[shape])
    B, T, F, H, K = shape
    assert empty_splits(B * (T + 1), 32) == [29, 30, 31] and (B * (T + 1) + 31) // 32 <= 29 * 7
    seed = SEEDS.get(("A", shape, which), 0)
    x, valid, y, _, wt = _problem(shape, seed)
    b = {"first": 0, "last": B - 1}.get(which)
    if b is None:
        b = _straddler(B, T, valid)
    assert valid[b, -1]
    w = np.zeros((B, T), np.float32)
    w[b, -3:] = (1.0, 0.5, 1.0)
    tag = "A %s one-%s-%s(b=%d)" % (mode, _sid(shape), which, b)

    def ref():
        _assert_margin(tag, x[b:b + 1], wt, K)
        return TR.loss_and_grads(x[b:b + 1], y[b:b + 1], w[b:b + 1], wt, K)
    sse_r, cnt_r, gr = _cached(("one", shape, which, seed), ref)
    assert cnt_r == 3.0 and all(np.abs(g).max() > 0 for g in gr)
    m = _model(dev, wt, K, "hard_sigmoid")
    sse, cnt, gs = _grads(m, dev, x, y, w)
    _check_loss(tag, sse, cnt, sse_r, cnt_r)
    _check(tag, gs, gr, _names(K))


def test_split_k_nan_workspace(dev, mode):
    """(33, 194) dense on a training workspace filled with NaN: bitwise the gradients of a fresh model -- the
    empty splits 29, 30, 31 store their zeros, nothing reads what it did not write."""
    from drnmf_amd import _capi
    shape = LONG[0]
    _assert_plan(shape, SPLIT_CASES[shape])
    B, T, F, H, K = shape
    x, _, y, w, wt = _problem(shape, sum(shape), flip=True)
    m = _model(dev, wt, K, "sigmoid")
    _, _, g0 = _grads(m, dev, x, y, w)
    m2 = _model(dev, wt, K, "sigmoid")
    need = _capi.lib().drnmf_lstm_train_workspace_bytes(ctypes.byref(m2._desc(B, T)))
    nan_ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=dev).view(torch.uint8)
    m2._train_ws = nan_ws
    _, _, g1 = _grads(m2, dev, x, y, w)
    assert nan_ws.numel() == need and m2._train_ws is nan_ws          # the run took place on that workspace
    for a, b, n in zip(g0, g1, _names(K)):
        assert np.isfinite(b).all(), n
        assert np.array_equal(a, b), n


# ---- B: the loss head alone (both modes) -------------------------------------------------------------------------

# (B, T, F): F across the 4-wide groups at 5 rows, B T = 1, 3, 4, 5, 1025 at F = 33 (and at F = 5): ceil(rows / 4)
# blocks of lstm_loss_rows_kernel = 1, 1, 1, 2 and 257 > the 256 threads of lstm_loss_final_kernel
HEAD_CASES = [(1, 5, F) for F in (1, 3, 4, 5, 33)] + [(1, 1, 33), (3, 1, 33), (2, 2, 33), (25, 41, 33), (25, 41, 5)]


@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "B%dT%dF%d" % c)
def test_loss_head_alone(dev, mode, case):
    """ops.lstm_loss_head_backward on a hidden tensor that is NOT the forward's (standard normal, times 1 and times
    8: saturated sigmoids), H = 13 and 16, rows contiguous (ld_h == H: with H = 13 the scalar paths of both GEMMs
    and the unpadded contraction) and padded to round_up(H, 4) with zeros in the padding columns, which is what
    include/drnmf_lstm.h says the forward leaves there.  Weights 0, 0.5 and 1, some on masked frames."""
    from drnmf_amd import ops
    B, T, F = case
    K = 1
    for H in (13, 16):
        rng = np.random.default_rng(1000 * F + 10 * B * T + H)
        x, valid = R.masked_input(rng, B, T, F)
        if B * T >= 4:                                           # more masked frames, anywhere but frame (0, 0)
            extra = rng.random((B, T)) < 0.3
            extra[0, 0] = False
            x[extra] = -1.0
            valid &= ~extra
        y = rng.random((B, T, F)).astype(np.float32)
        w = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=(B, T))
        w[0, 0] = 0.5
        if B * T > 1000:
            assert (w[~valid] != 0).any() and (w[valid] == 0).any() and (~valid).sum() > 100
        wt = R.random_weights(rng, F, H, K)
        desc = ops.make_lstm_desc(B, T, F, H, K)
        params = ops.lstm_prepare_params(desc, [_dv(wt[0], dev)], [_dv(wt[1], dev)], [_dv(wt[2], dev)],
                                         _dv(wt[3], dev), _dv(wt[4], dev))
        ws = ops.lstm_train_workspace(desc, dev)
        ops.lstm_train_forward(_dv(x, dev), -1.0, params, desc, ws)       # the head reads xm from the workspace
        xm = x * valid[..., None]
        for scale in (1.0, 8.0):
            hid = (scale * rng.standard_normal((B, T, H))).astype(np.float32)
            ref = _cached(("head", case, H, scale),
                          lambda: TR.head_loss_and_grads(xm, hid, y, w, wt[3], wt[4]))
            layouts = {"contiguous": _dv(hid, dev)}
            if H % 4:
                buf = torch.zeros((B, T, _rup(H, 4)), dtype=torch.float32, device=dev)
                buf[..., :H] = _dv(hid, dev)
                layouts["padded"] = buf[..., :H]
            for lname, hd in sorted(layouts.items()):
                sums = torch.full((2,), float("nan"), device=dev)
                d_h = torch.full((B, T, H), float("nan"), device=dev)
                d_wo = torch.full((H, F), float("nan"), device=dev)
                d_bo = torch.full((F,), float("nan"), device=dev)
                ops.lstm_loss_head_backward(_dv(y, dev), _dv(w, dev), hd, params, _dv(wt[3], dev), desc, ws, sums,
                                            d_h, d_wo, d_bo)
                torch.cuda.synchronize()
                tag = "B %s B%dT%dF%dH%d-x%d-%s" % (mode, B, T, F, H, scale, lname)
                s = sums.cpu().numpy()
                _check_loss(tag, float(s[0]), float(s[1]), ref[0], ref[1])
                _check(tag, [d_h.cpu().numpy(), d_wo.cpu().numpy(), d_bo.cpu().numpy()], ref[2:],
                       ["d_hidden", "d_w_out", "d_b_out"])


# ---- C: the BPTT alone (f32 mode) --------------------------------------------------------------------------------

class Chain(object):
    """Training forward + drnmf_lstm_backward on one workspace and one set of buffers (so that every call replays
    the same cached graphs), the cotangent supplied by the caller."""

    def __init__(self, dev, x, wt, K, act, state=None):
        from drnmf_amd import ops
        B, T, F = x.shape
        H = wt[1].shape[0]
        self.dev, self.K, self.x = dev, K, _dv(x, dev)
        self.w = [_dv(a, dev) for a in wt]
        self.desc = ops.make_lstm_desc(B, T, F, H, K, act)
        self.params = ops.lstm_prepare_params(self.desc, self.w[0:3 * K:3], self.w[1:3 * K:3], self.w[2:3 * K:3],
                                              self.w[-2], self.w[-1])
        self.ws = ops.lstm_train_workspace(self.desc, dev)
        self.hid = torch.empty((B, T, _rup(H, 4)), dtype=torch.float32, device=dev)[..., :H]
        self.d_hidden = torch.empty((B, T, H), dtype=torch.float32, device=dev)
        self.state = None if state is None else tuple(_dv(s, dev) for s in state)
        self.g = [torch.empty_like(a) for a in self.w[:3 * K]]

    def vjp(self, cot, run_head=False):
        """A fresh forward (the backward overwrites z in place), then the BPTT from `cot`.  run_head: the loss head
        in between, its d_hidden then overwritten by `cot`."""
        from drnmf_amd import ops
        K, w, g = self.K, self.w, self.g
        ops.lstm_train_forward(self.x, -1.0, self.params, self.desc, self.ws, out=self.hid,
                               initial_state=self.state)
        if run_head:
            B, T, F = self.x.shape
            ops.lstm_loss_head_backward(torch.rand((B, T, F), device=self.dev), torch.ones((B, T), device=self.dev),
                                        self.hid, self.params, w[-2], self.desc, self.ws,
                                        torch.empty(2, device=self.dev), self.d_hidden, torch.empty_like(w[-2]),
                                        torch.empty_like(w[-1]))
        self.d_hidden.copy_(_dv(cot, self.dev))
        for t in g:
            t.fill_(float("nan"))
        ops.lstm_backward(w[0:3 * K:3], w[1:3 * K:3], self.d_hidden, g[0::3], g[1::3], g[2::3], self.desc, self.ws)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in g]


@pytest.fixture
def f32(dev):
    with _matrix_mode("f32", dev) as m:
        yield m


BPTT_SHAPE = (17, 12, 9, 37)          # B (two 16-row tiles, every mask pattern twice), T, F, H (two 32-unit tiles)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("K", [1, 3])
def test_bptt_alone(dev, f32, K, act):
    """ops.lstm_backward on cotangents that no loss head produces, against hidden_vjp."""
    B, T, F, H = BPTT_SHAPE
    seed = SEEDS.get(("C", K), 0)
    x, valid, _, _, wt = _problem((B, T, F, H, K), seed)
    tag = "C f32 K%d-%s" % (K, act)
    if act == "hard_sigmoid":
        _assert_margin(tag, x, wt, K)
    names = _names(K)[:3 * K]
    rng = np.random.default_rng(K)
    ch = Chain(dev, x, wt, K, act)
    ref = lambda c: TR.hidden_vjp(x, wt, K, c, -1.0, act)

    dense = rng.standard_normal((B, T, H)).astype(np.float32)
    g = ch.vjp(dense)
    _check(tag + " dense", g, ref(dense), names)
    g2 = ch.vjp(dense, run_head=True)            # the head between the two changes nothing the BPTT reads
    for a, b in zip(g, g2):
        assert np.array_equal(a, b)

    masked = dense * ~valid[..., None]           # nothing on a valid frame: all of it is carried ph
    assert (~valid).sum() > B and (masked != 0).any()
    _check(tag + " masked-frames-only", ch.vjp(masked), ref(masked), names)

    allm = np.nonzero(~valid.any(axis=1))[0]     # the all-masked rows (one per 16-row tile): exactly nothing
    assert list(allm) == [5, 12]
    c = np.zeros_like(dense)
    c[allm] = dense[allm]
    for a, n in zip(ch.vjp(c), names):
        assert not a.any(), "%s all-masked rows %s: gradient not exactly zero" % (tag, n)

    for b in (0, 15, 16):                        # 16 = B - 1: the one row of the second tile
        for t in (0, T - 1):
            c = np.zeros_like(dense)
            c[b, t] = 1.0
            r = ref(c)
            g = ch.vjp(c)
            t_eff = [u for u in range(t + 1) if valid[b, u]]
            if not t_eff:                        # a masked frame with no valid frame before it
                for a, n in zip(g, names):
                    assert not a.any(), "%s impulse (%d, %d) %s: not exactly zero" % (tag, b, t, n)
                assert not any(a.any() for a in r)
                continue
            _check("%s impulse(b=%d,t=%d,lands=%d)" % (tag, b, t, t_eff[-1]), g, r, names)
    assert not valid[15, T - 1] and valid[15, 0] and not valid[16, 0] and valid[16, T - 1]


def test_bptt_alone_with_an_entering_state(dev, f32):
    """The entering state (h, c of magnitude about 1) is a constant of the gradient: c_{-1} in dz_f of frame 0,
    h_{-1} in the recurrent-kernel gradient; rows masked from frame 0 on carry their gradient to nothing."""
    B, T, F, H = BPTT_SHAPE
    K = 3
    x, valid, _, _, wt = _problem((B, T, F, H, K), 3)
    rng = np.random.default_rng(33)
    st = SR.random_state(rng, K, B, H)
    ch = Chain(dev, x, wt, K, "sigmoid", state=st)
    names = _names(K)[:3 * K]
    dense = rng.standard_normal((B, T, H)).astype(np.float32)
    for what, c in (("dense", dense), ("masked-frames-only", dense * ~valid[..., None])):
        _check("C f32 K3-state " + what, ch.vjp(c), TR.hidden_vjp(x, wt, K, c, -1.0, "sigmoid", st), names)


# ---- D: graph chunks of the two training chains (both modes) -----------------------------------------------------

# (T, K) -> frames = (T + K) // 2: 63 (one graph), 64 with a dead half-frame (127 diagonals), exactly 64,
# 64 + 1 remainder, 64 + 37 remainders
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("T,K", [(126, 1), (127, 1), (128, 1), (129, 1), (200, 3)], ids=lambda v: str(v))
def test_training_graph_chunks(dev, mode, monkeypatch, T, K, act):
    """Full gradients across the chunking of the training forward (counter going up) and the BPTT (counter going
    down from T + K - 2); the cached graphs a second time (the counters restart); at (129, 1) and (200, 3) the
    same launches made directly."""
    shape = (3, T, 9, 10, K)
    assert (T + K) // 2 == {126: 63, 127: 64, 128: 64, 129: 65, 200: 101}[T]
    tag = "D %s T%dK%d-%s" % (mode, T, K, act)
    m, (x, _, y, w, _), g1, _ = _full_case(dev, tag, shape, act, seed=T + K,
                                           scale=0.5 if act == "hard_sigmoid" else 1.5)
    _, _, g2 = _grads(m, dev, x, y, w)
    for a, b, n in zip(g1, g2, _names(K)):
        assert np.array_equal(a, b), "second replay differs: " + n
    if T in (129, 200):
        monkeypatch.setenv("DRNMF_NO_GRAPH", "1")
        _, _, g3 = _grads(m, dev, x, y, w)
        monkeypatch.delenv("DRNMF_NO_GRAPH")
        for a, b, n in zip(g1, g3, _names(K)):
            assert np.array_equal(a, b), "direct launches differ from the graphs: " + n


# ---- E: tile edges, one dimension at a time ----------------------------------------------------------------------

BASE = (5, 6, 9, 10, 2)


def _vary(**kw):
    d = dict(zip("BTFHK", BASE))
    d.update(kw)
    return tuple(d[c] for c in "BTFHK")


# H across the 8-unit forward tiles and the 32-unit BPTT tiles, B across the 16-row tiles, F across the 4-bin groups
# and one 64-lane pass of the row kernels, T = 1 (K = 1: a single diagonal), K > T
EDGE_SHAPES = [_vary(H=H) for H in (1, 7, 8, 9, 16, 17, 31, 32, 33, 64, 65)] + \
    [_vary(B=B) for B in (1, 15, 16, 17, 32, 33)] + [_vary(F=F) for F in (1, 3, 4, 5, 64, 65)] + \
    [_vary(T=1, K=1), _vary(T=1, K=3), _vary(T=2, K=5)]
EDGE_X3 = [_vary(H=33), _vary(B=17), _vary(F=5), _vary(T=1, K=3), _vary(T=2, K=5)]


@pytest.mark.parametrize("shape,mm", [(s, "f32") for s in EDGE_SHAPES] + [(s, "bf16x3") for s in EDGE_X3],
                         ids=lambda v: v if isinstance(v, str) else _sid(v))
def test_tile_edges(dev, shape, mm):
    """Gradients, loss and test_on_batch at BASE with one dimension moved; the activation alternates."""
    act = ACTS[sum(shape) % 2]
    with _matrix_mode(mm, dev):
        _full_case(dev, "E %s %s-%s" % (mm, _sid(shape), act), shape, act, seed=SEEDS.get(("E", shape), 0),
                   test_loss=True)


# ---- F: mask values ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask_value", [0.0, None], ids=["zero", "none"])
@pytest.mark.parametrize("act", ACTS)
def test_mask_values(dev, mode, mask_value, act):
    """mask_value 0.0: a frame of zeros is masked (and single zero bins are input).  None: no frame is masked -- the
    frames of -1 that tests/lstm_ref.py's masked_input writes are input and every frame counts in the loss."""
    shape = (7, 9, 20, 13, 2)
    tag = "F %s mask-%s-%s" % (mode, mask_value, act)
    _, (x, valid, _, w, _), _, _ = _full_case(dev, tag, shape, act, seed=SEEDS.get(("F", mask_value), 0),
                                              mask_value=mask_value, test_loss=True)
    if mask_value is None:
        assert valid.all() and (x == -1.0).all(axis=-1).any()
    else:
        assert (x[~valid] == 0.0).all() and (~valid).any() and (w[~valid] != 0).any()
