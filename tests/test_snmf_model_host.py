"""CPU-side tests of the sparse-NMF baseline as a model: the C ABI of include/drnmf_snmf.h (exports, binding,
admission rule, workspace query, argument validation on an unbound handle), the argument checks and the weight
surface of layers.SparseNMFModel, and two properties of the fp64 reference the GPU tests lean on (no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import snmf_model_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_snmf.h")
NAMES = {"drnmf_snmf_mask_admitted", "drnmf_snmf_mask_workspace_bytes", "drnmf_snmf_mask_forward"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


def test_snmf_header_is_plain_c_and_matches_the_binding(capi, tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(drnmf_[a-z0-9_]+)\s*\(", src))
    assert declared == NAMES
    assert declared == set(capi.SNMF_SIGNATURES), declared ^ set(capi.SNMF_SIGNATURES)
    for other in (capi.SIGNATURES, capi.LSTM_SIGNATURES, capi.SCORE_SIGNATURES, capi.ENHANCE_SIGNATURES,
                  capi.SDR_SIGNATURES, capi.DATASET_SIGNATURES, capi.STREAM_SIGNATURES):
        assert not (declared & set(other))
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(HDR).read()) == ["drnmf.h"]
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "drnmf_snmf.h":
            assert "drnmf_snmf_mask" not in open(os.path.join(ROOT, "include", name)).read(), name
    L = capi.lib()
    for name in sorted(declared):
        fn = getattr(L, name)                 # exported ...
        assert fn.argtypes == capi.SNMF_SIGNATURES[name][1]          # ... and bound by _capi.lib()
        assert fn.restype == capi.SNMF_SIGNATURES[name][0]
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "no C compiler"
    c = tmp_path / "snmf_header_check.c"
    c.write_text('#include "drnmf_snmf.h"\ntypedef void (*fn_t)(void);\nstatic const fn_t refs[] = {\n' +
                 "".join("    (fn_t)%s,\n" % n for n in sorted(declared)) +
                 "};\nint main(void) { return refs[0] != 0 ? 0 : 1; }\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(c)], check=True)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in doc, name


def test_admission_rule_and_workspace_query(capi):
    L = capi.lib()
    adm = L.drnmf_snmf_mask_admitted
    assert adm(257, 512, 2.0) == 1 and adm(257, 200, 2.0) == 1 and adm(5, 10, 2.0) == 1
    assert adm(257, 514, 2.0) == 0 and adm(257, 200, 1.0) == 0 and adm(257, 200, 1.5) == 0
    q = L.drnmf_snmf_mask_workspace_bytes
    for bad in ((0, 7, 129, 200), (3, 0, 129, 200), (3, 7, 0, 200), (3, 7, 129, 0), (3, 7, 129, 201)):
        assert q(*bad) == 0, bad
    sizes = [q(B, T, 129, 200) for B, T in ((1, 1), (1, 17), (3, 7), (2, 16), (4, 250), (250, 250))]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] > 0      # monotone in B * T
    assert q(3, 7, 129, 200) == q(7, 3, 129, 200) and q(3, 7, 129, 200) % 256 == 0
    # V, H and drnmf_mu_forward's own buffers at the very least
    assert q(3, 7, 129, 200) >= 21 * (129 + 200) * 4 + L.drnmf_mu_workspace_bytes(21, 129, 200)


def test_forward_validates_before_it_touches_a_device(capi):
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(B=1, T=1, F=5, N=10, n_iter=3, beta=2.0, sparsity=0.1, power=1.0, has_mask=1, x=p, Wn=p, h0=p, out=p,
             path=2):
        return L.drnmf_snmf_mask_forward(h, B, T, F, N, n_iter, beta, sparsity, power, -1.0, has_mask, x, Wn, h0, out,
                                         path, None, 0, None)
    try:
        for bad in (dict(N=11), dict(B=0), dict(T=0), dict(F=0), dict(N=0), dict(n_iter=-1), dict(path=3),
                    dict(path=-1), dict(sparsity=-1.0), dict(has_mask=2), dict(x=None), dict(Wn=None), dict(h0=None),
                    dict(out=None)):
            assert call(**bad) == -1, bad
            assert L.drnmf_last_error(h)
        assert call(N=514) == -2 and b"514" in L.drnmf_last_error(h)        # DRNMF_ERR_UNSUPPORTED: tile path only
        assert call(beta=1.0) == -2
        assert call(N=514, path=1) == -4 and call(N=514, path=0) == -4     # the GEMM path wants its workspace
        assert call(path=1) == -4
        # path = 0 switches to the GEMM path (which wants its workspace) above the measured row count the binding
        # mirrors; at or below it the tile kernel is launched, which a handle without a device cannot do
        rows = capi.SNMF_TILE_AUTO_MAX_ROWS
        assert call(B=1, T=rows + 1, path=0) == -4
        assert call(B=1, T=rows, path=0) == -3
    finally:
        L.drnmf_destroy(h)


def _model(**kw):
    from drnmf_amd import layers
    _, W, h_init = R.problem(3, 7, 129, 200)
    args = dict(W=W, r=100, sparsity=0.1, device="cpu")
    args.update(kw)
    return layers.SparseNMFModel(**args)


def test_model_argument_errors(capi):
    import torch
    from drnmf_amd import layers, ops
    _, W, h_init = R.problem(3, 7, 129, 200)
    with pytest.raises(ValueError, match="2r"):
        _model(W=W[:, :199], r=100)                               # odd N
    with pytest.raises(ValueError, match="2r"):
        _model(W=W[:, :198], r=100)                               # N != 2 r
    with pytest.raises(ValueError, match="h_init"):
        _model(h_init=h_init[:-1])
    with pytest.raises(ValueError, match="path"):
        _model(path="fast")
    with pytest.raises(ValueError):
        _model(n_iter=-1)
    m = _model(h_init=h_init)
    assert m._input_width() == 129 and m._output_width() == 129 and m._stateful() and not m._carries_state()
    assert m.reset_states(batch_size=4) is None and m.n_iter == 200 and m.beta == 2.0
    with pytest.raises(ValueError, match="129"):                  # W rows != F of the input
        m.forward(torch.zeros(1, 3, 128))
    with pytest.raises(ValueError):
        m.set_weights([W[:-1]])
    x = torch.zeros(1, 3, 129)
    Wt, ht = torch.from_numpy(W), torch.from_numpy(h_init)
    with pytest.raises(ValueError, match="shape"):
        ops.snmf_mask_forward(x, Wt[:-1], ht, 0.1, 3)
    with pytest.raises(ValueError, match="shape"):
        ops.snmf_mask_forward(x, Wt, ht[:-1], 0.1, 3)
    with pytest.raises(ValueError, match="even"):
        ops.snmf_mask_forward(x, Wt[:, :199], ht[:199], 0.1, 3)
    with pytest.raises(ValueError, match="path"):
        ops.snmf_mask_forward(x, Wt, ht, 0.1, 3, path="fast")
    for call in (m.compile, m.fit):
        with pytest.raises(NotImplementedError, match="from_wavs"):
            call()
    b = layers.build_snmf(dict(r=100, sparsity=1., cf="ed", random_seed=2016., max_iter=1000., conv_eps=1e-4,
                               display=0.), W, device="cpu")
    assert (b.r, b.sparsity, b.n_iter, b.beta, b.spectrogram_power, b.path) == (100, 1.0, 200, 2.0, 1.0, "auto")
    np.testing.assert_array_equal(b.h_init.numpy(), np.random.RandomState(2016).rand(200).astype(np.float32))
    assert layers.build_snmf(dict(r=100, cf="kl", spectrogram_power=2.), W, device="cpu").beta == 1.0
    rows = capi.SNMF_TILE_AUTO_MAX_ROWS
    assert ops.snmf_mask_path("auto", rows, 129, 200) == "tile" and ops.snmf_mask_path("auto", rows + 1, 129, 200) == "gemm"
    assert ops.snmf_mask_path("auto", 16, 129, 514) == "gemm" and ops.snmf_mask_path("auto", 16, 129, 200, 1.0) == "gemm"
    assert ops.snmf_mask_path("tile", 10 ** 6, 129, 200) == "tile" and ops.snmf_mask_path("gemm", 1, 129, 200) == "gemm"


def test_weights_and_the_normalised_copy(capi, tmp_path):
    _, W, h_init = R.problem(3, 7, 129, 200)
    m = _model(h_init=h_init)
    assert [w.shape for w in m.get_weights()] == [(129, 200)]
    Wn, hn = m._operands()
    want_W, want_h = R.normalised(W, h_init)
    np.testing.assert_allclose(Wn.numpy(), want_W, rtol=1e-6)
    np.testing.assert_allclose(hn.numpy(), want_h, rtol=1e-6)
    np.testing.assert_allclose((Wn.numpy().astype(np.float64) ** 2).sum(axis=0), 1.0, rtol=1e-6)
    assert m._operands()[0] is Wn                                 # kept while W stays
    path = str(tmp_path / "w.npz")
    m.save_weights(path)
    tree = m.weights_tree()
    assert list(tree["layer_names"]) == ["snmf_dictionary"] and list(tree["snmf_dictionary/weight_names"]) == ["W"]
    m.set_weights([2 * W[:, ::-1]])
    Wn2, hn2 = m._operands()                                      # remade when W changes
    np.testing.assert_allclose(Wn2.numpy(), want_W[:, ::-1], rtol=1e-6)
    np.testing.assert_allclose(hn2.numpy(), 2 * R.normalised(W[:, ::-1], h_init)[1], rtol=1e-6)
    m.load_weights(path)
    np.testing.assert_array_equal(m.get_weights()[0], W)
    np.testing.assert_allclose(m._operands()[0].numpy(), want_W, rtol=1e-6)


def test_reference_frames_together_equal_frames_alone():
    """What the shared h_init buys: in the fp64 reference a recording's frames run together are the same frames
    run one at a time.  (Equal up to the BLAS kernel numpy picks for one column or many: a few ulp of fp64.)"""
    B, T, F, N = 3, 7, 129, 200
    x, W, h_init = R.problem(B, T, F, N)
    together = R.case_reference(B, T, F, N)
    alone = np.zeros_like(together)
    for b in range(B):
        for t in range(T):
            alone[b, t] = R.reference_mask(x[b:b + 1, t:t + 1], W, h_init, R.SPARSITY, R.N_ITER)[0, 0]
    assert np.max(np.abs(together - alone)) <= 1e-12
    assert not together[2].any() and not together[1, 4:].any() and together[1, :4].all()


@pytest.mark.parametrize("case", R.CASES + [R.WIDE])
def test_reference_masks_are_not_trivial(case):
    """A constant mask would pass any comparison: over the valid frames of every GPU case the reference spreads."""
    B, T, F, N = case
    ref = R.case_reference(B, T, F, N)
    v = ref[R.valid_frames(B, T)]
    assert v.size and v.min() >= 0 and v.max() <= 1
    assert v.std() > 0.05 and v.max() - v.min() > 0.3, (v.std(), v.min(), v.max())
