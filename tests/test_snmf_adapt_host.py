"""CPU-side tests of the noise-adaptive sparse-NMF baseline: the numpy reference tests/snmf_adapt_ref.py against the
oracle's training loop and on the three rules it adds, the C ABI of include/drnmf_snmf_adapt.h (exports, binding,
workspace query, argument validation on an unbound handle) and the model's option (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

import snmf_adapt_ref as A
from oracle import drnmf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_snmf_adapt.h")
NAMES = {"drnmf_snmf_adapt_admitted", "drnmf_snmf_adapt_workspace_bytes", "drnmf_snmf_adapt_forward"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


def _problem(T, F, N, n0, seed=3):
    rng = np.random.RandomState(seed)
    W = rng.rand(F, N) + 0.05
    Wn = W / np.sqrt((W * W).sum(0))
    x = (rng.rand(T, F) + 0.01).astype(np.float32)
    h = rng.rand(N)
    return x, Wn, h


@pytest.mark.parametrize("T,F,N,n0,n_iter,power", [(1, 5, 10, 5, 30, 1.0), (37, 33, 48, 24, 30, 1.0),
                                                   (20, 17, 12, 0, 10, 2.0), (20, 17, 12, 12, 10, 1.0),
                                                   (9, 33, 50, 19, 0, 1.0)])
def test_reference_is_the_oracle_where_no_rule_fires(T, F, N, n0, n_iter, power):
    x, Wn, h = _problem(T, F, N, n0)
    V = x.astype(np.float64) ** power
    W64, H64, _ = O.sparse_nmf_train(V.T, Wn, np.tile(h[:, None], (1, T)), 0.1, n_iter, conv_eps=0, beta=2,
                                     w_update_ind=(np.arange(N) >= n0))
    want = O.snmf_irm(W64, H64, N // 2).T
    mask, W, H = A.adapt_forward(x[None], Wn, h, 0.1, n_iter, n0, power=power)
    assert np.abs(mask[0] - want).max() <= 1e-12
    assert np.abs(W[0] - W64).max() <= 1e-12
    assert np.abs(H[0] - H64.T).max() <= 1e-12 * max(1.0, np.abs(H64).max())
    assert np.array_equal(W[0][:, :n0], Wn[:, :n0])                      # rule 1
    if n0 < N and n_iter:
        assert np.abs(np.sqrt((W[0][:, n0:] ** 2).sum(0)) - 1).max() <= 1e-12
        assert np.abs(W[0][:, n0:] - Wn[:, n0:]).max() > 1e-3            # the noise atoms did move


def test_rules_on_a_silent_row_an_empty_row_and_one_frame():
    T, F, N, n0 = 6, 9, 8, 4
    x, Wn, h = _problem(T, F, N, n0)
    xb = np.stack([x, np.zeros_like(x), np.full_like(x, -1.0), x])
    xb[3, 1:] = -1.0                                                     # T = 1: one valid frame
    mask, W, H = A.adapt_forward(xb, Wn, h, 0.1, 5, n0)
    assert np.isfinite(mask).all() and np.isfinite(W).all() and np.isfinite(H).all()
    # rule 2: the silent row is valid (0 != mask_value); its numerator is 0, every new column would be 0 / 0
    assert np.array_equal(W[1], Wn) and np.all(H[1] == 0) and np.all(mask[1] == 0)
    with np.errstate(all="ignore"):
        Wo, _, _ = O.sparse_nmf_train(np.zeros((F, T)), Wn, np.tile(h[:, None], (1, T)), 0.1, 5, conv_eps=0,
                                      beta=2, w_update_ind=(np.arange(N) >= n0))
    assert np.isnan(Wo[:, n0:]).all()                                    # what the oracle makes of it
    # rule 3: no valid frame
    assert np.array_equal(W[2], Wn) and np.all(mask[2] == 0) and np.all(H[2] == 0)
    # one frame: the row alone, whatever lies behind it
    m1, W1, H1 = A.adapt_forward(x[None, :1], Wn, h, 0.1, 5, n0)
    assert np.array_equal(m1[0, 0], mask[3, 0]) and np.array_equal(W1[0], W[3])
    assert np.all(mask[3, 1:] == 0) and np.all(H[3, 1:] == 0)
    # n_iter = 0: the mask of h_init and Wn
    m0, W0, H0 = A.adapt_forward(x[None], Wn, h, 0.1, 0, n0)
    assert np.array_equal(W0[0], Wn) and np.array_equal(H0[0], np.tile(h, (T, 1)))
    assert np.abs(m0[0] - O.snmf_irm(Wn, np.tile(h[:, None], (1, T)), N // 2).T).max() <= 1e-15


def test_header_and_binding(capi):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(drnmf_[a-z0-9_]+)\s*\(", src))
    assert declared == NAMES == set(capi.SNMF_ADAPT_SIGNATURES)
    L = capi.lib()
    for name in sorted(declared):
        fn = getattr(L, name)                                            # exported and bound
        assert fn.argtypes == capi.SNMF_ADAPT_SIGNATURES[name][1]
        assert fn.restype == capi.SNMF_ADAPT_SIGNATURES[name][0]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in doc, name


def test_admission_and_workspace_query(capi):
    L = capi.lib()
    adm = L.drnmf_snmf_adapt_admitted
    assert adm(257, 200, 2.0) == 1 and adm(5, 2, 2.0) == 1 and adm(257, 512, 2.0) == 1
    assert adm(257, 514, 2.0) == 0 and adm(257, 1, 2.0) == 0 and adm(257, 200, 1.0) == 0 and adm(0, 200, 2.0) == 0
    q = L.drnmf_snmf_adapt_workspace_bytes
    for bad in [(0, 10, 33, 48, 24), (2, 0, 33, 48, 24), (2, 10, 0, 48, 24), (2, 10, 33, 0, 0), (2, 10, 33, 47, 3),
                (2, 10, 33, 514, 2), (2, 10, 33, 48, -1), (2, 10, 33, 48, 49), (65536, 10, 33, 48, 24)]:
        assert q(*bad) == 0, bad
    B, T, F, N, n0 = 3, 70, 33, 48, 24
    need = q(B, T, F, N, n0)
    nblk = -(-T // 64)
    floor = 4 * (B * F * N + B * T * N + B * T + B * nblk + B * nblk * 2 * F * (N - n0))
    assert floor <= need <= floor + 5 * 256 and need % 256 == 0
    assert q(B, T, F, N, N) < q(B, T, F, N, n0) < q(B, T, F, N, 0)       # the partials grow with the updated atoms


def test_forward_validates_before_it_touches_a_device(capi):
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)
        B, T, F, N, n0 = 2, 10, 33, 48, 24
        need = L.drnmf_snmf_adapt_workspace_bytes(B, T, F, N, n0)

        def call(B=B, T=T, F=F, N=N, n0=n0, n_iter=3, sparsity=0.1, has_mask=1, x=fake, Wn=fake, hi=fake,
                 out=fake, ws=fake, nbytes=need, handle=h):
            return L.drnmf_snmf_adapt_forward(handle, B, T, F, N, n0, n_iter, sparsity, 1.0, -1.0, has_mask, x, Wn,
                                              hi, out, None, None, ws, nbytes, None)
        err = lambda: L.drnmf_last_error(h)
        assert call(handle=None) == -1
        for kw, word in [(dict(B=0), b"bad shape"), (dict(T=-1), b"bad shape"), (dict(n_iter=-1), b"bad shape"),
                         (dict(N=47), b"even"), (dict(n0=-1), b"n0"), (dict(n0=49), b"n0"),
                         (dict(B=65536), b"65535"), (dict(sparsity=-0.5), b"sparsity"),
                         (dict(sparsity=float("nan")), b"sparsity"), (dict(has_mask=2), b"has_mask"),
                         (dict(x=None), b"NULL"), (dict(Wn=None), b"NULL"), (dict(hi=None), b"NULL"),
                         (dict(out=None), b"NULL")]:
            assert call(**kw) == -1, kw                                  # DRNMF_ERR_INVALID_ARG
            assert word in err(), (kw, err())
        assert call(N=514, n0=2) == -2 and b"512" in err()               # DRNMF_ERR_UNSUPPORTED
        assert call(nbytes=need - 1) == -4 and b"workspace" in err()     # DRNMF_ERR_WORKSPACE
        assert call(ws=None) == -4
        # everything in order: what stops the call is that the handle is bound to no device
        rc = call()
        assert rc not in (0, -1, -2, -4) and b"no device" in err()
    finally:
        L.drnmf_destroy(h)


def _model(**kw):
    from drnmf_amd import layers
    W = np.random.RandomState(0).rand(33, 2 * kw.pop("r", 8)).astype(np.float32) + 0.05
    args = dict(W=W, r=W.shape[1] // 2, sparsity=0.1, device="cpu")
    args.update(kw)
    return layers.SparseNMFModel(**args)


def test_model_option(capi):
    from drnmf_amd import layers
    assert _model().adapt_noise is False
    m = _model(adapt_noise=True)
    assert m.adapt_noise is True
    for kw in (dict(operand_dtype="float16"), dict(beta=1.0), dict(r=257), dict(path="gemm")):
        with pytest.raises(ValueError, match="adapt_noise"):
            _model(adapt_noise=True, **kw)
        if "r" not in kw and "operand_dtype" not in kw:
            _model(**kw)                                                 # fine without the option
    with pytest.raises(NotImplementedError, match="adapt"):
        m.stream(2)
    W = np.random.RandomState(0).rand(33, 16).astype(np.float32) + 0.05
    assert layers.build_snmf(dict(r=8, cf="ed", adapt_noise=True), W, device="cpu").adapt_noise is True
    assert layers.build_snmf(dict(r=8, cf="ed"), W, device="cpu").adapt_noise is False
    # the weight surface is the fixed model's
    assert [w.shape for w in m.get_weights()] == [(33, 16)]
    assert np.array_equal(m.get_weights()[0], _model().get_weights()[0])
