"""CPU-side tests of the online noise-adaptive sparse-NMF baseline: the numpy reference tests/snmf_online_ref.py against
the oracle and on the rules it adds, the C ABI of include/drnmf_snmf_online.h (exports, binding, the byte queries,
argument validation on an unbound handle) and the model's option (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

import snmf_online_ref as Q
from oracle import drnmf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_snmf_online.h")
NAMES = {"drnmf_snmf_online_admitted", "drnmf_snmf_online_state_bytes", "drnmf_snmf_online_workspace_bytes",
         "drnmf_snmf_online_reset", "drnmf_snmf_online_forward", "drnmf_snmf_online_read"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


def _problem(T, F, N, seed=3):
    rng = np.random.RandomState(seed)
    W = rng.rand(F, N) + 0.05
    Wn = W / np.sqrt((W * W).sum(0))
    x = (rng.rand(T, F) + 0.01).astype(np.float32)
    h = rng.rand(N)
    return x, Wn, h


# ---- the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,F,N,n0,L,n_iter,power", [(1, 5, 10, 5, 16, 30, 1.0), (37, 33, 48, 24, 48, 30, 1.0),
                                                     (20, 17, 12, 0, 32, 10, 2.0), (9, 33, 50, 19, 16, 0, 1.0)])
def test_first_block_is_mu_infer_and_snmf_irm(T, F, N, n0, L, n_iter, power):
    """With L >= the frame count no block fills: every frame is the oracle's inference on Wn."""
    x, Wn, h = _problem(T, F, N)
    V = x.astype(np.float64) ** power
    H64, _ = O.mu_infer(V.T, Wn, np.tile(h[:, None], (1, T)), 0.1, n_iter, beta=2.0)
    want = O.snmf_irm(Wn, H64, N // 2).T
    mask, H, rows = Q.online_forward(x[None], Wn, h, 0.1, n_iter, n0, L, power=power)
    assert np.abs(mask[0] - want).max() <= 1e-12
    assert np.abs(H[0] - H64.T).max() <= 1e-12 * max(1.0, np.abs(H64).max())
    assert np.array_equal(rows[0].W, Wn) and rows[0].count == T and not rows[0].A.any() and not rows[0].blocks
    if n_iter == 0:
        assert np.array_equal(H[0], np.tile(h, (T, 1)))                  # the mask of h_init


@pytest.mark.parametrize("T,F,N,n0", [(16, 5, 10, 5), (32, 33, 48, 24), (48, 17, 12, 0)])
def test_one_iteration_on_one_block_is_one_iteration_of_the_oracles_training(T, F, N, n0):
    """n_iter = 1, w_iter = 1, L = T, forget = 1: no clamp fires on these inputs, so W (H^T H_u) = Lambda^T H_u and the
    dictionary after the first block is the oracle's after one iteration."""
    x, Wn, h = _problem(T, F, N)
    W64, H64, _ = O.sparse_nmf_train(x.astype(np.float64).T, Wn, np.tile(h[:, None], (1, T)), 0.1, 1, conv_eps=0,
                                     beta=2, w_update_ind=(np.arange(N) >= n0))
    _, H, rows = Q.online_forward(x[None], Wn, h, 0.1, 1, n0, T)
    assert rows[0].count == T and len(rows[0].blocks) == 1 and not rows[0].V
    assert np.abs(rows[0].W - W64).max() <= 1e-12
    assert np.abs(H[0] - H64.T).max() <= 1e-12 * max(1.0, np.abs(H64).max())
    assert np.array_equal(rows[0].W[:, :n0], Wn[:, :n0])                 # rule 1
    assert np.abs(rows[0].W[:, n0:] - Wn[:, n0:]).max() > 1e-3           # the noise atoms did move
    assert np.abs(np.sqrt((rows[0].W[:, n0:] ** 2).sum(0)) - 1).max() <= 1e-12


def test_w_iter_0_and_all_atoms_fixed_never_move_w():
    T, F, N = 40, 9, 8
    x, Wn, h = _problem(T, F, N)
    fixed_mask, fixed_H, _ = Q.online_forward(x[None], Wn, h, 0.1, 5, 4, 64)         # one unfilled block: Wn throughout
    for kw in (dict(n0=4, w_iter=0), dict(n0=N, w_iter=2)):
        mask, H, rows = Q.online_forward(x[None], Wn, h, 0.1, 5, kw["n0"], 16, w_iter=kw["w_iter"])
        assert np.array_equal(rows[0].W, Wn) and rows[0].count == T and len(rows[0].blocks) == 2
        assert np.array_equal(mask, fixed_mask) and np.array_equal(H, fixed_H)
    _, _, rows = Q.online_forward(x[None], Wn, h, 0.1, 5, 4, 16, w_iter=0)
    assert rows[0].A.any() and rows[0].Bm.any()                          # the statistics are kept all the same


def test_rules_on_a_silent_row_an_empty_row_and_an_unfilled_block():
    T, F, N, n0, L = 40, 9, 8, 4, 16
    x, Wn, h = _problem(T, F, N)
    xb = np.stack([x, np.zeros_like(x), np.full_like(x, -1.0), x])
    xb[3, 15:] = -1.0                                                    # 15 valid frames: the block never fills
    mask, H, rows = Q.online_forward(xb, Wn, h, 0.1, 5, n0, L)
    assert np.isfinite(mask).all() and np.isfinite(H).all() and all(np.isfinite(r.W).all() for r in rows)
    assert [r.count for r in rows] == [40, 40, 0, 15]
    assert len(rows[0].blocks) == 2 and len(rows[0].V) == 8 and np.abs(rows[0].W - Wn).max() > 1e-3
    # rule 2: the silent row is valid (0 != mask_value); its statistics are 0 and every new column would be 0 / 0
    assert np.array_equal(rows[1].W, Wn) and len(rows[1].blocks) == 2 and not H[1].any() and not mask[1].any()
    # no valid frame: nothing happens
    assert np.array_equal(rows[2].W, Wn) and not mask[2].any() and not H[2].any() and not rows[2].V
    # an unfilled block causes no update, and its frames are the first block's of row 0
    assert np.array_equal(rows[3].W, Wn) and not rows[3].A.any() and len(rows[3].V) == 15
    assert np.array_equal(mask[3, :15], mask[0, :15]) and not mask[3, 15:].any() and not H[3, 15:].any()
    # interior masked frames are skipped and not counted: the row with them removed
    gone = np.zeros(T, bool)
    gone[[0, 5, 6, 17, 39]] = True
    xm = x.copy()
    xm[gone] = -1.0
    m1, H1, r1 = Q.online_forward(xm[None], Wn, h, 0.1, 5, n0, L)
    m2, H2, r2 = Q.online_forward(x[None, ~gone], Wn, h, 0.1, 5, n0, L)
    assert np.array_equal(m1[0, ~gone], m2[0]) and np.array_equal(H1[0, ~gone], H2[0])
    assert not m1[0, gone].any() and np.array_equal(r1[0].W, r2[0].W) and r1[0].count == r2[0].count == 35


def test_the_reference_does_not_depend_on_the_cuts():
    T, F, N, n0, L = 70, 9, 8, 4, 16
    x, Wn, h = _problem(T, F, N)
    kw = dict(w_iter=2, forget=0.9)
    mask, H, rows = Q.online_forward(x[None], Wn, h, 0.1, 5, n0, L, **kw)
    state, at, pm, pH = None, 0, [], []
    for n in (1, 15, 16, 17, 3, 0, 18):
        m, hh, state = Q.online_forward(x[None, at:at + n], Wn, h, 0.1, 5, n0, L, rows=state, **kw)
        pm.append(m[0])
        pH.append(hh[0])
        at += n
    assert at == T
    assert np.array_equal(np.concatenate(pm), mask[0]) and np.array_equal(np.concatenate(pH), H[0])
    a, b = state[0], rows[0]
    assert np.array_equal(a.W, b.W) and np.array_equal(a.A, b.A) and np.array_equal(a.Bm, b.Bm)
    assert a.count == b.count == T and len(a.V) == len(b.V) == T % L


@pytest.mark.parametrize("n_iter", [30, 200])
def test_later_blocks_fit_the_unseen_noise_better_than_the_fixed_dictionary(n_iter):
    """On mixtures whose noise the dictionary has not seen, every block after the first has a lower divergence
    sum (V - W H)^2 than the same frames on the fixed dictionary."""
    T, F, N, n0, L = 160, 33, 48, 24, 16
    x, Wn, h = Q.mixture(1, T, F, N, n0)
    Wn, h = Wn.astype(np.float64), h.astype(np.float64)
    _, _, rows = Q.online_forward(x, Wn, h, 0.1, n_iter, n0, L)
    _, Hf, _ = Q.online_forward(x, Wn, h, 0.1, n_iter, N, L)
    assert len(rows[0].blocks) == T // L
    ratios = []
    for k, (Vb, Hb, Wk) in enumerate(rows[0].blocks):
        fixed = Q.divergence(Vb, Wn, Hf[0, k * L:(k + 1) * L])
        ratios.append(Q.divergence(Vb, Wk, Hb) / fixed)
    print("divergence against the fixed dictionary's, per block:", " ".join("%.3f" % r for r in ratios))
    assert abs(ratios[0] - 1) <= 1e-12                                    # the first block runs on Wn
    assert all(r < 1 for r in ratios[1:])


# ---- the ABI ------------------------------------------------------------------------------------------------------
def test_header_and_binding(capi):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(drnmf_[a-z0-9_]+)\s*\(", src))
    assert declared == NAMES == set(capi.SNMF_ONLINE_SIGNATURES)
    L = capi.lib()
    for name in sorted(declared):
        fn = getattr(L, name)                                            # exported and bound
        assert fn.argtypes == capi.SNMF_ONLINE_SIGNATURES[name][1]
        assert fn.restype == capi.SNMF_ONLINE_SIGNATURES[name][0]
    # the argument counts of the header's declarations
    for name, body in re.findall(r"\b(drnmf_snmf_online_[a-z_]+)\s*\(([^)]*)\)", src):
        assert len(body.split(",")) == len(capi.SNMF_ONLINE_SIGNATURES[name][1]), name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES | {"SNMF_ONLINE_SIGNATURES", "SNMF_ONLINE_MAX_N", "snmf_online_state", "snmf_online_workspace",
                         "snmf_online_forward", "snmf_online_dictionaries", "adapt_block", "adapt_forget",
                         "adapt_w_iter"}:
        assert name in doc, name
    assert capi.SNMF_ONLINE_MAX_N == 512


def test_admission_and_byte_queries(capi):
    L = capi.lib()
    adm = L.drnmf_snmf_online_admitted
    assert adm(257, 200, 2.0, 64) == 1 and adm(5, 2, 2.0, 16) == 1 and adm(257, 512, 2.0, 256) == 1
    for bad in [(257, 514, 2.0, 64), (257, 1, 2.0, 64), (257, 47, 2.0, 64), (257, 200, 1.0, 64), (0, 200, 2.0, 64),
                (257, 200, 2.0, 0), (257, 200, 2.0, 24), (257, 200, 2.0, 272), (257, 200, 2.0, -16)]:
        assert adm(*bad) == 0, bad
    qs, qw = L.drnmf_snmf_online_state_bytes, L.drnmf_snmf_online_workspace_bytes
    for bad in [(0, 33, 48, 24, 16), (2, 0, 48, 24, 16), (2, 33, 0, 0, 16), (2, 33, 47, 3, 16), (2, 33, 514, 2, 16),
                (2, 33, 48, -1, 16), (2, 33, 48, 49, 16), (65536, 33, 48, 24, 16), (2, 33, 48, 24, 0),
                (2, 33, 48, 24, 24), (2, 33, 48, 24, 272)]:
        assert qs(*bad) == 0, bad
        assert qw(bad[0], 10, *bad[1:]) == 0, bad
    assert qw(2, 0, 33, 48, 24, 16) == 0
    B, T, F, N, n0, blk = 3, 70, 33, 48, 24, 32
    Nu = N - n0
    need = qs(B, F, N, n0, blk)
    floor = 8 * B + 4 * B * (F * N + N * Nu + F * Nu + blk * F + blk * N)
    assert floor <= need <= floor + 6 * 256 and need % 256 == 0
    assert qs(B, F, N, N, blk) < need < qs(B, F, N, 0, blk) and need < qs(B, F, N, n0, 64)
    work = qw(B, T, F, N, n0, blk)
    floor = 4 * (2 * B * T + 2 * B + B * blk + B * blk * F + 2 * B * F * Nu)
    assert floor <= work <= floor + 8 * 256 and work % 256 == 0
    assert work < qw(B, 2 * T, F, N, n0, blk)


def test_entries_validate_before_they_touch_a_device(capi):
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)
        B, T, F, N, n0, blk = 2, 10, 33, 48, 24, 16
        sneed = L.drnmf_snmf_online_state_bytes(B, F, N, n0, blk)
        wneed = L.drnmf_snmf_online_workspace_bytes(B, T, F, N, n0, blk)

        def call(B=B, T=T, F=F, N=N, n0=n0, block=blk, n_iter=3, w_iter=1, sparsity=0.1, forget=1.0, has_mask=1,
                 x=fake, hi=fake, out=fake, st=fake, sbytes=sneed, ws=fake, wbytes=wneed, handle=h):
            return L.drnmf_snmf_online_forward(handle, B, T, F, N, n0, block, n_iter, w_iter, sparsity, forget, 1.0,
                                               -1.0, has_mask, x, hi, out, None, st, sbytes, ws, wbytes, None)
        err = lambda: L.drnmf_last_error(h)
        assert call(handle=None) == -1
        for kw, word in [(dict(B=0), b"bad shape"), (dict(T=-1), b"bad shape"), (dict(n_iter=-1), b"bad shape"),
                         (dict(N=47), b"even"), (dict(n0=-1), b"n0"), (dict(n0=49), b"n0"),
                         (dict(B=65536), b"65535"), (dict(block=0), b"block"), (dict(block=24), b"block"),
                         (dict(block=272), b"block"), (dict(w_iter=-1), b"w_iter"), (dict(forget=0.0), b"forget"),
                         (dict(forget=1.5), b"forget"), (dict(forget=float("nan")), b"forget"),
                         (dict(sparsity=-0.5), b"sparsity"), (dict(sparsity=float("nan")), b"sparsity"),
                         (dict(has_mask=2), b"has_mask"), (dict(x=None), b"NULL"), (dict(hi=None), b"NULL"),
                         (dict(out=None), b"NULL")]:
            assert call(**kw) == -1, kw                                  # DRNMF_ERR_INVALID_ARG
            assert word in err(), (kw, err())
        assert call(N=514, n0=2) == -2 and b"512" in err()               # DRNMF_ERR_UNSUPPORTED
        assert call(sbytes=sneed - 1) == -4 and b"state" in err()        # DRNMF_ERR_WORKSPACE
        assert call(st=None) == -4 and b"state" in err()
        assert call(st=ctypes.c_void_p(0x100010)) == -4 and b"aligned" in err()
        assert call(wbytes=wneed - 1) == -4 and b"workspace" in err()
        assert call(ws=None) == -4
        # everything in order: what stops the call is that the handle is bound to no device
        rc = call()
        assert rc not in (0, -1, -2, -4) and b"no device" in err()

        def reset(B=B, F=F, N=N, n0=n0, block=blk, Wn=fake, st=fake, sbytes=sneed):
            return L.drnmf_snmf_online_reset(h, B, F, N, n0, block, Wn, None, st, sbytes, None)

        def read(B=B, F=F, N=N, n0=n0, block=blk, st=fake, sbytes=sneed):
            return L.drnmf_snmf_online_read(h, B, F, N, n0, block, st, sbytes, fake, None, None, None, None)
        for fn in (reset, read):
            for kw in (dict(B=0), dict(N=47), dict(n0=49), dict(block=24), dict(block=272)):
                assert fn(**kw) == -1, (fn.__name__, kw)
            assert fn(N=514, n0=2) == -2
            assert fn(sbytes=sneed - 1) == -4 and fn(st=None) == -4
            rc = fn()
            assert rc not in (0, -1, -2, -4) and b"no device" in err()
        assert reset(Wn=None) == -1 and b"NULL" in err()
    finally:
        L.drnmf_destroy(h)


# ---- the model's option ---------------------------------------------------------------------------------------------
def _model(**kw):
    from drnmf_amd import layers
    W = np.random.RandomState(0).rand(33, 2 * kw.pop("r", 8)).astype(np.float32) + 0.05
    args = dict(W=W, r=W.shape[1] // 2, sparsity=0.1, device="cpu")
    args.update(kw)
    return layers.SparseNMFModel(**args)


def test_model_option(capi):
    from drnmf_amd import layers
    fixed, batch, online = _model(), _model(adapt_noise=True), _model(adapt_noise="online")
    assert fixed.adapt_noise is False and batch.adapt_noise is True and online.adapt_noise == "online"
    assert (online.adapt_block, online.adapt_forget, online.adapt_w_iter) == (64, 1.0, 1)
    assert [m._carries_state() for m in (fixed, batch, online)] == [False, False, True]
    assert all(m._stateful() for m in (fixed, batch, online))
    for kw in (dict(operand_dtype="float16"), dict(beta=1.0), dict(r=257), dict(path="gemm")):
        with pytest.raises(ValueError, match="adapt_noise='online'"):
            _model(adapt_noise="online", **kw)
    for kw in (dict(adapt_block=0), dict(adapt_block=24), dict(adapt_block=272), dict(adapt_forget=0.0),
               dict(adapt_forget=1.5), dict(adapt_forget=float("nan")), dict(adapt_w_iter=-1),
               dict(adapt_w_iter=1.5)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            _model(adapt_noise="online", **kw)
    with pytest.raises(ValueError, match="adapt_noise"):
        _model(adapt_noise="offline")
    m = _model(adapt_noise="online", adapt_block=16, adapt_forget=0.9, adapt_w_iter=0, path="tile")
    assert (m.adapt_block, m.adapt_forget, m.adapt_w_iter) == (16, 0.9, 0)
    # the batch mode still does not stream; the fixed model has no dictionaries to show; enhance regroups rows
    with pytest.raises(NotImplementedError, match="adapt"):
        batch.stream(2)
    for other in (fixed, batch):
        with pytest.raises(ValueError, match="online"):
            other.dictionaries()
    with pytest.raises(NotImplementedError, match="stateful"):
        online.enhance([np.zeros(2000, np.int16)], N=64, hop=16)
    online.reset_states()                                                # nothing bound yet: nothing to do
    W = np.random.RandomState(0).rand(33, 16).astype(np.float32) + 0.05
    b = layers.build_snmf(dict(r=8, cf="ed", adapt_noise="online", adapt_block=32, adapt_forget=0.5, adapt_w_iter=4),
                          W, device="cpu")
    assert b.adapt_noise == "online" and (b.adapt_block, b.adapt_forget, b.adapt_w_iter) == (32, 0.5, 4)
    assert layers.build_snmf(dict(r=8, cf="ed", adapt_noise="online"), W, device="cpu").adapt_block == 64
    assert layers.build_snmf(dict(r=8, cf="ed", adapt_noise=True), W, device="cpu").adapt_noise is True
    assert layers.build_snmf(dict(r=8, cf="ed"), W, device="cpu").adapt_noise is False
    # the weight surface is the fixed model's
    assert [w.shape for w in online.get_weights()] == [(33, 16)]
    assert np.array_equal(online.get_weights()[0], fixed.get_weights()[0])
