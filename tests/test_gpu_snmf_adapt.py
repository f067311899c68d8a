"""The noise-adaptive sparse-NMF baseline on the GPU (csrc/snmf_adapt.hip, ops.snmf_adapt_forward,
SparseNMFModel(adapt_noise=True)) against the fp64 numpy reference tests/snmf_adapt_ref.py.

Inputs: a speech part W[:, :n0] Hs plus a noise part from a dictionary the model has not seen, activations about 30 %
non-zero, W = rand + 0.05, one shared h_init, sparsity 0.1.  Bounds: the mask MSE is the project's MASK_MSE_TOL; the
dictionary is held to max(8 e32, 1e-6) max|W64|, e32 being the relative error of the same numpy reference run in
float32 on the same input (the factor 8 covers the MFMA summation order differing from BLAS's); the per-row
divergence to 1e-4 relative.  Everything about rows being independent is bitwise."""
import numpy as np
import pytest
import torch

import snmf_adapt_ref as A
import snmf_model_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPARSITY, MASK_VALUE = 0.1, -1.0
# (B, T, F, N, n0) -> the rows' valid lengths (None: all T)
SHAPES = {(1, 1, 5, 10, 5): None, (4, 37, 33, 48, 24): (37, 17, 1, 0), (2, 33, 33, 50, 19): None,
          (2, 70, 129, 200, 100): None, (2, 40, 257, 512, 256): None, (2, 20, 33, 48, 0): None,
          (2, 20, 33, 48, 48): None}
# (shape, n_iter, power)
CASES = [(s, 30, 1.0) for s in SHAPES] + [((2, 70, 129, 200, 100), 200, 1.0), ((2, 70, 129, 200, 100), 30, 2.0)]


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def problem(shape, seed=11):
    B, T, F, N, n0 = shape
    lengths = SHAPES.get(shape) or (T,) * B
    rng = np.random.RandomState(seed)
    W = rng.rand(F, N) + 0.05
    D = rng.rand(F, max(N - n0, N // 2)) + 0.05                  # the noise of the recordings: not in W
    h_init = rng.rand(N)
    x = np.full((B, T, F), MASK_VALUE, np.float32)
    for b, n in enumerate(lengths):
        Hs = rng.rand(n, n0) * (rng.rand(n, n0) < 0.3)
        Hn = rng.rand(n, D.shape[1]) * (rng.rand(n, D.shape[1]) < 0.3)
        x[b, :n] = Hs @ W[:, :n0].T + Hn @ D.T
    nrm = np.sqrt((W * W).sum(0))
    Wn = (W / nrm).astype(np.float32)
    return x, Wn, (h_init * nrm).astype(np.float32)


_REF = {}


def reference(shape, n_iter, power, dtype=np.float64, n0=None):
    """(mask, W, H) of the numpy reference, computed once per key and never changed."""
    key = (shape, n_iter, power, np.dtype(dtype).name, n0)
    if key not in _REF:
        x, Wn, hn = problem(shape)
        out = A.adapt_forward(x, Wn.astype(np.float64), hn.astype(np.float64), SPARSITY, n_iter,
                              shape[4] if n0 is None else n0, power=power, mask_value=MASK_VALUE, dtype=dtype)
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def run(ops, x, Wn, hn, n_iter, n0, power=1.0):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    m, W, H = ops.snmf_adapt_forward(t(x), t(Wn), t(hn), SPARSITY, n_iter, n0, power=power, mask_value=MASK_VALUE,
                                     return_dictionaries=True, return_activations=True)
    return m.cpu().numpy(), W.cpu().numpy(), H.cpu().numpy()


@pytest.mark.parametrize("shape,n_iter,power", CASES)
def test_against_the_reference(ops, shape, n_iter, power):
    B, T, F, N, n0 = shape
    x, Wn, hn = problem(shape)
    m, W, H = run(ops, x, Wn, hn, n_iter, n0, power)
    m64, W64, H64 = reference(shape, n_iter, power)
    _, W32, _ = reference(shape, n_iter, power, dtype=np.float32)
    _, Wf, Hf = reference(shape, n_iter, power, n0=N)             # the fixed dictionary on the same rows
    valid = np.any(x != MASK_VALUE, axis=-1)
    assert np.isfinite(m).all() and np.isfinite(W).all() and np.isfinite(H).all()
    assert not m[~valid].any() and not H[~valid].any(), "masked frames must be exactly 0"
    mse = float(np.mean((m - m64) ** 2))
    scale = float(np.abs(W64).max())
    e32 = float(np.abs(W32 - W64).max()) / scale
    dW = float(np.abs(W - W64).max())
    print("snmf adapt %s it %d power %g: mask MSE %.3e, max|dW| %.3e (bound %.3e, e32 %.3e)"
          % (shape, n_iter, power, mse, dW, max(8 * e32, 1e-6) * scale, e32))
    assert mse <= R.MASK_MSE_TOL
    assert dW <= max(8 * e32, 1e-6) * scale
    assert np.array_equal(W[:, :, :n0], np.broadcast_to(Wn[:, :n0], (B, F, n0)))      # fixed atoms: the bits of Wn
    for b in range(B):
        if not valid[b].any():
            assert np.array_equal(W[b], Wn)
            continue
        if n0 < N and n_iter:
            assert np.abs(np.sqrt((W[b][:, n0:].astype(np.float64) ** 2).sum(0)) - 1).max() <= 1e-6
        V = x[b][valid[b]].astype(np.float64) ** power
        d = A.divergence(V, W[b], H[b][valid[b]])
        d64 = A.divergence(V, W64[b], H64[b][valid[b]])
        dfix = A.divergence(V, Wf[b], Hf[b][valid[b]])
        print("  row %d: divergence %.6e, reference %.6e, fixed dictionary %.6e" % (b, d, d64, dfix))
        assert abs(d - d64) <= 1e-4 * d64
        if valid[b].sum() > 1 and n0 < N and n_iter:
            assert d < dfix and d64 < dfix


@pytest.mark.parametrize("path", ["tile", "gemm"])
def test_all_atoms_fixed_is_the_fixed_model(ops, path):
    shape = (2, 20, 33, 48, 48)
    x, Wn, hn = problem(shape)
    m, W, _ = run(ops, x, Wn, hn, 30, 48)
    t = lambda a: torch.from_numpy(a).to(DEV)
    want = ops.snmf_mask_forward(t(x), t(Wn), t(hn), SPARSITY, 30, mask_value=MASK_VALUE, path=path).cpu().numpy()
    assert np.abs(m - want).max() <= 1e-5
    assert np.array_equal(W, np.broadcast_to(Wn, W.shape))


def test_rows_do_not_depend_on_batch_position_or_padding(ops):
    """Bitwise: every row of the ragged batch alone, at another position, and with T padded from 37 to 64; a silent
    row beside them leaves with the dictionary it came with."""
    shape = (4, 37, 33, 48, 24)
    x, Wn, hn = problem(shape)
    whole = run(ops, x, Wn, hn, 30, 24)
    for b in range(4):
        alone = run(ops, x[b:b + 1], Wn, hn, 30, 24)
        for a, w in zip(alone, whole):
            assert np.array_equal(a[0], w[b]), b
    order = [2, 0, 3, 1]
    moved = run(ops, x[order], Wn, hn, 30, 24)
    for a, w in zip(moved, whole):
        assert np.array_equal(a, w[order])
    xp = np.full((5, 64, 33), MASK_VALUE, np.float32)
    xp[:4, :37] = x
    xp[4, :9] = 0.0                                               # digitally silent, but valid
    m, W, H = run(ops, xp, Wn, hn, 30, 24)
    assert np.array_equal(m[:4, :37], whole[0]) and np.array_equal(W[:4], whole[1])
    assert np.array_equal(H[:4, :37], whole[2])
    assert not m[:, 37:].any() and not H[:, 37:].any()
    assert np.array_equal(W[4], Wn) and np.isfinite(m[4]).all() and not H[4].any()


def test_interior_masked_frames(ops):
    """Masked frames inside a row: the result is that of the row with those frames removed (to rounding: the other
    frames move to other places in the order of the sums)."""
    shape = (2, 70, 129, 200, 100)
    x, Wn, hn = problem(shape)
    x = x[:1].copy()
    gone = np.zeros(70, bool)
    gone[[0, 5, 6, 7, 31, 32, 63, 64, 69]] = True
    xm = x.copy()
    xm[0, gone] = MASK_VALUE
    m, W, H = run(ops, xm, Wn, hn, 30, 100)
    ms, Ws, Hs = run(ops, x[:, ~gone], Wn, hn, 30, 100)
    assert not m[0, gone].any() and not H[0, gone].any()
    assert np.abs(m[0, ~gone] - ms[0]).max() <= 1e-5
    assert np.abs(W - Ws).max() <= 1e-5


# ---- the model ---------------------------------------------------------------------------------------------------
N_M, HOP_M, F_M = 256, 64, 129


def _model(adapt=True, n_iter=30):
    from drnmf_amd import layers
    rng = np.random.RandomState(4)
    W = (rng.rand(F_M, 200) + 0.05).astype(np.float32)
    return layers.SparseNMFModel(W, 100, SPARSITY, n_iter=n_iter, h_init=rng.rand(200), device=DEV,
                                 adapt_noise=adapt)


def _recordings():
    rng = np.random.default_rng(5)
    return [(rng.standard_normal(n) * 3000 * (1 + 0.5 * np.sin(np.arange(n) / 700.0))).astype(np.int16)
            for n in (1500, 2317, 900)]


def test_model_forward_is_the_op_and_leaves_the_weights(ops):
    m = _model()
    before = m.get_weights()[0].copy()
    x = torch.from_numpy(problem((2, 70, 129, 200, 100))[0]).to(DEV)
    mask, Wd = m.forward(x, return_dictionaries=True)
    Wn, hn = m._operands()
    want, Wwant = ops.snmf_adapt_forward(x, Wn, hn, SPARSITY, 30, 100, mask_value=MASK_VALUE, return_dictionaries=True)
    assert torch.equal(mask, want) and torch.equal(Wd, Wwant) and tuple(Wd.shape) == (2, F_M, 200)
    assert torch.equal(m.forward(x), want)
    assert float((Wd[:, :, 100:] - Wn[:, 100:]).abs().max()) > 1e-3          # the noise atoms moved
    assert np.array_equal(m.get_weights()[0], before)
    with pytest.raises(NotImplementedError):
        m.stream(1, N=N_M, hop=HOP_M)
    fixed = _model(adapt=False)
    assert torch.equal(fixed.forward(x), ops.snmf_mask_forward(x, Wn, hn, SPARSITY, 30, mask_value=MASK_VALUE))
    with pytest.raises(ValueError, match="adapt_noise"):
        fixed.forward(x, return_dictionaries=True)


def test_predict_in_slabs_equals_forward_row_by_row(ops):
    m = _model()
    p = problem((2, 70, 129, 200, 100))[0][:, :23]
    x = np.stack([p[0], p[1], p[0][::-1], p[1], p[0]]).copy()      # five rows, ragged
    x[1, 17:] = MASK_VALUE
    x[2, 5:] = MASK_VALUE
    x[3, :] = MASK_VALUE
    x[4, 22:] = MASK_VALUE
    got = m.predict(x, batch_size=2)
    rows = np.concatenate([m.forward(torch.from_numpy(x[i:i + 1]).to(DEV)).cpu().numpy() for i in range(5)])
    assert np.array_equal(got, rows)
    assert np.array_equal(m.predict_on_batch(x), rows)
    masked = ~np.any(x != MASK_VALUE, axis=-1)
    assert not got[masked].any() and got[~masked].std() > 0        # (a constant mask would make the above empty)


def test_enhance_equals_the_stages_by_hand(ops):
    m = _model()
    wavs = _recordings()
    lens = [len(w) for w in wavs]
    pcm = np.zeros((len(wavs), max(lens)), np.int16)
    for i, w in enumerate(wavs):
        pcm[i, :len(w)] = w
    x, re, im, nf = ops.stft_ragged(torch.from_numpy(pcm).to(DEV), lens, N=N_M, hop=HOP_M, mask_value=MASK_VALUE)
    mask = m.forward(x)
    y = ops.istft_ragged(re, im, mask, lens, N_M, HOP_M, crop=True).cpu().numpy()
    got, masks = m.enhance(wavs, N=N_M, hop=HOP_M, dtype="float32", crop=True, return_masks=True, batch_size=2)
    for i, n in enumerate(lens):
        assert np.array_equal(got[i], y[i, :n]), i                 # bitwise: rows are independent
        assert np.array_equal(masks[i], mask[i, :int(nf[i])].cpu().numpy())
    clean = [(0.8 * w).astype(np.int16) for w in wavs]
    out, S, labels = m.enhance(wavs, N=N_M, hop=HOP_M, ref=clean)
    assert len(out) == 3 and np.asarray(S).shape == (3, 6)
    # val_loss: one row per recording, the fixed model's formula over the same frames
    p = m.spectrogram_power
    yc = ops.stft_ragged(torch.from_numpy(np.stack([np.pad(c, (0, max(lens) - len(c))) for c in clean])).to(DEV),
                         lens, N=N_M, hop=HOP_M, mask_value=MASK_VALUE)[0]
    keep = (torch.arange(x.shape[1], device=DEV)[None] < torch.from_numpy(nf).to(DEV)[:, None])[..., None]
    want = float(torch.where(keep, (mask * x ** p - yc ** p) ** 2, torch.zeros_like(x)).sum() / (int(nf.sum()) * F_M))
    assert abs(m.val_loss(wavs, clean, N=N_M, hop=HOP_M) - want) <= 1e-6 * want
