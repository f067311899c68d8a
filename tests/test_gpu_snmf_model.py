"""The sparse-NMF baseline as a model on the MI355X (csrc/snmf_mask.hip, layers.SparseNMFModel): both paths of
drnmf_snmf_mask_forward against the fp64 reference of tests/snmf_model_ref.py (oracle.mu_infer + oracle.snmf_irm per
valid frame, one shared initial vector), the tile kernel's bitwise independence of a row from its position and
its neighbours, and the model surface (predict, enhance, stream, from_wavs).

Cases (B, T, F, N), 30 iterations, sparsity 0.1:
  (1, 1, 5, 10)      one row in a padded tile; F below a 32-bin chunk; N below a 16-column tile
  (1, 17, 33, 48)    two tiles, the second padded; one bin past a chunk
  (3, 7, 129, 200)   ragged lengths with one all-masked sequence; tiles straddling sequences
  (2, 9, 257, 512)   masked frames in the interior; the admission edge (the wide form of the kernel)
The entry exposes the mask only (H stays on chip), so the bound is the project's mask bound, MASK_MSE_TOL."""
import ctypes

import numpy as np
import pytest
import torch

import snmf_model_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_M, HOP_M, F_M = 256, 64, 129          # the model-level tests: a small model, N = 200 atoms


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _run(ops, case, path, beta=2.0, power=1.0, n_iter=R.N_ITER):
    x, W, h_init = R.problem(*case)
    Wn, hn = R.normalised(W, h_init)
    t = lambda a: torch.from_numpy(a).to(DEV)
    out = ops.snmf_mask_forward(t(x), t(Wn), t(hn), R.SPARSITY, n_iter, beta=beta, power=power,
                                mask_value=R.MASK_VALUE, path=path)
    return out.cpu().numpy()


def _check(got, case, what, **ref_kw):
    ref = R.case_reference(*case, **ref_kw)
    valid = R.valid_frames(case[0], case[1])
    mse = float(np.mean((got - ref) ** 2))
    print("snmf mask %s %s: MSE %.3e, max |d| %.3e" % (case, what, mse, float(np.max(np.abs(got - ref)))))
    assert np.isfinite(got).all()
    assert not got[~valid].any(), "masked rows must be exactly 0"
    assert mse <= R.MASK_MSE_TOL, (case, what, mse)


@pytest.mark.parametrize("path", ["tile", "gemm"])
@pytest.mark.parametrize("case", R.CASES)
def test_mask_against_the_reference(ops, case, path):
    _check(_run(ops, case, path), case, path)


@pytest.mark.parametrize("path", ["tile", "gemm"])
def test_spectrogram_power_two(ops, path):
    case = (3, 7, 129, 200)
    _check(_run(ops, case, path, power=2.0), case, path + " power 2", power=2.0)


def test_shapes_the_tile_kernel_does_not_take(ops):
    """path = 2 at N = 514 is DRNMF_ERR_UNSUPPORTED; path = 0 there, and at beta = 1, runs the GEMM path."""
    from drnmf_amd import _capi
    x, W, h_init = R.problem(*R.WIDE)
    Wn, hn = R.normalised(W, h_init)
    xd, Wd, hd = (torch.from_numpy(a).to(DEV) for a in (x, Wn, hn))
    out = torch.empty_like(xd)
    B, T, F, N = R.WIDE
    rc = _capi.lib().drnmf_snmf_mask_forward(_capi.handle(0), B, T, F, N, R.N_ITER, 2.0, R.SPARSITY, 1.0,
                                             R.MASK_VALUE, 1, _capi.ptr(xd), _capi.ptr(Wd), _capi.ptr(hd),
                                             _capi.ptr(out), 2, None, 0, ctypes.c_void_p(0))
    assert rc == -2
    with pytest.raises(ValueError, match="tile kernel"):
        ops.snmf_mask_forward(xd, Wd, hd, R.SPARSITY, R.N_ITER, mask_value=R.MASK_VALUE, path="tile")
    _check(_run(ops, R.WIDE, "auto"), R.WIDE, "auto at N = 514")
    case = (3, 7, 129, 200)
    _check(_run(ops, case, "auto", beta=1.0), case, "auto at beta = 1", beta=1.0)


def test_auto_rule_follows_the_row_count(ops):
    """path = 0 is the tile kernel up to _capi.SNMF_TILE_AUTO_MAX_ROWS rows and the GEMM path beyond: the same bits
    as the path it names (a small dictionary keeps the GEMM run just above the row count short)."""
    from drnmf_amd import _capi
    rows = _capi.SNMF_TILE_AUTO_MAX_ROWS
    _, W, h_init = R.problem(1, 1, 5, 10)
    Wn, hn = R.normalised(W, h_init)
    Wd, hd = torch.from_numpy(Wn.copy()).to(DEV), torch.from_numpy(hn.copy()).to(DEV)
    x = torch.rand((1, rows + 1, 5), generator=torch.Generator().manual_seed(1)).to(DEV) + 0.01
    run = lambda v, p: ops.snmf_mask_forward(v.contiguous(), Wd, hd, R.SPARSITY, 5, mask_value=R.MASK_VALUE, path=p)
    assert torch.equal(run(x, "auto"), run(x, "gemm"))
    assert torch.equal(run(x[:, :rows], "auto"), run(x[:, :rows], "tile"))
    assert float((run(x, "tile") - run(x, "gemm")).abs().max()) <= 1e-5


def test_tile_rows_do_not_depend_on_position_or_neighbours(ops):
    """Bitwise: the mask of (3, 7, 129, 200) equals the masks of the same rows run one sequence at a time and one
    frame at a time (a row moves through every position of a tile, beside valid, masked and padding rows)."""
    case = (3, 7, 129, 200)
    x, W, h_init = R.problem(*case)
    Wn, hn = R.normalised(W, h_init)
    xd, Wd, hd = (torch.from_numpy(a).to(DEV) for a in (x, Wn, hn))
    run = lambda v: ops.snmf_mask_forward(v.contiguous(), Wd, hd, R.SPARSITY, R.N_ITER, mask_value=R.MASK_VALUE,
                                          path="tile")
    whole = run(xd)
    by_seq = torch.cat([run(xd[b:b + 1]) for b in range(case[0])])
    by_frame = torch.cat([torch.cat([run(xd[b:b + 1, t:t + 1]) for t in range(case[1])], dim=1)
                          for b in range(case[0])])
    assert torch.equal(whole, by_seq)
    assert torch.equal(whole, by_frame)
    shifted = run(torch.cat([xd[2:], xd[:2]]))                    # the same rows 7 positions further on
    assert torch.equal(whole, torch.cat([shifted[1:], shifted[:1]]))


# ---- the model ---------------------------------------------------------------------------------------------------
def _model(n_iter=R.N_ITER, path="tile"):
    from drnmf_amd import layers
    _, W, h_init = R.problem(3, 7, F_M, 200)
    return layers.SparseNMFModel(W, 100, R.SPARSITY, n_iter=n_iter, h_init=h_init, path=path, device=DEV)


def _recordings():
    rng = np.random.default_rng(5)
    return [(rng.standard_normal(n) * 3000 * (1 + 0.5 * np.sin(np.arange(n) / 700.0))).astype(np.int16)
            for n in (1500, 2317, 900)]


def test_default_iteration_count_against_the_reference(ops):
    """n_iter = 200, the reference's inference setting (enhance.py:842), through model.forward."""
    from drnmf_amd import layers
    case = (3, 7, 129, 200)
    x, W, h_init = R.problem(*case)
    for path in ("tile", "gemm"):
        m = layers.SparseNMFModel(W, 100, R.SPARSITY, h_init=h_init, path=path, device=DEV)
        assert m.n_iter == 200
        got = m.forward(torch.from_numpy(x).to(DEV)).cpu().numpy()
        _check(got, case, path + " 200 iterations", n_iter=200)


def test_predict_in_slabs_equals_forward_row_by_row(ops):
    m = _model()
    p = R.problem(3, 7, F_M, 200)[0]
    x = np.stack([p[0], p[1], p[2], p[0][::-1], p[1]]).copy()      # 5 sequences: ragged, one all masked
    x[4, :3] = R.MASK_VALUE                                        # ... and one that starts masked
    got = m.predict(x, batch_size=2)
    rows = np.concatenate([m.forward(torch.from_numpy(x[i:i + 1]).to(DEV)).cpu().numpy() for i in range(5)])
    assert np.array_equal(got, rows)                               # bitwise: frames are independent
    assert np.array_equal(m.predict_on_batch(x), rows)
    masked = ~np.any(x != R.MASK_VALUE, axis=-1)
    assert masked.any() and not got[masked].any() and got[~masked].std() > 0.05


def test_enhance_equals_the_stages_by_hand(ops):
    m = _model()
    wavs = _recordings()
    lens = [len(w) for w in wavs]
    pcm = np.zeros((len(wavs), max(lens)), np.int16)
    for i, w in enumerate(wavs):
        pcm[i, :len(w)] = w
    x, re, im, nf = ops.stft_ragged(torch.from_numpy(pcm).to(DEV), lens, N=N_M, hop=HOP_M, mask_value=R.MASK_VALUE)
    mask = m.forward(x)
    y = ops.istft_ragged(re, im, mask, lens, N_M, HOP_M, crop=True).cpu().numpy()
    got, masks = m.enhance(wavs, N=N_M, hop=HOP_M, dtype="float32", crop=True, return_masks=True)
    for i, n in enumerate(lens):
        assert got[i].shape == (n,)
        assert np.array_equal(got[i], y[i, :n]), i                 # bitwise: same kernels, independent frames
        assert np.array_equal(masks[i], mask[i, :int(nf[i])].cpu().numpy())
    clean = [(0.8 * w).astype(np.int16) for w in wavs]
    out, S, labels = m.enhance(wavs, N=N_M, hop=HOP_M, ref=clean)
    assert len(out) == 3 and out[0].dtype == np.int16
    assert np.asarray(S).shape == (3, 6) and len(labels) == 6


def test_stream_equals_the_whole_recording(ops):
    """model.stream over uneven chunks (empty ones included) against the whole recordings: the comparison of
    tests/test_gpu_stream.py (1e-4 of the peak, 5 int16 steps); the float32 samples are in fact bitwise."""
    from test_gpu_stream import _model_schedules, _push_all
    m = _model()
    wavs = _recordings()
    lens = [len(w) for w in wavs]
    rf = m.enhance(wavs, N=N_M, hop=HOP_M, dtype="float32", crop=True)
    pcm = np.zeros((len(wavs), max(lens)), np.int16)
    for i, w in enumerate(wavs):
        pcm[i, :len(w)] = w
    x, re, im, nf = ops.stft_ragged(torch.from_numpy(pcm).to(DEV), lens, N=N_M, hop=HOP_M, mask_value=R.MASK_VALUE)
    yr = ops.istft_ragged(re, im, m.forward(x), lens, N_M, HOP_M, crop=True)
    rq = ops.to_int16_wav_rows(yr, lens).cpu().numpy()
    for name, sch in _model_schedules(wavs).items():
        yf = _push_all(m.stream(len(wavs), N=N_M, hop=HOP_M, dtype="float32", crop=True), wavs, sch)
        yq = _push_all(m.stream(len(wavs), N=N_M, hop=HOP_M, dtype="int16", crop=True), wavs, sch)
        for i, n in enumerate(lens):
            assert yf[i].shape == (n,) and yq[i].shape == (n,)
            df = float(np.max(np.abs(yf[i] - rf[i])) / np.max(np.abs(rf[i])))
            dq = int(np.max(np.abs(yq[i].astype(np.int32) - rq[i, :n].astype(np.int32))))
            bitwise = np.array_equal(yf[i], rf[i])
            print("snmf stream %s row %d: float32 %.3e of the peak (bitwise %s), int16 %d" % (name, i, df, bitwise, dq))
            assert df <= 1e-4 and dq <= 5, (name, i, df, dq)
            assert bitwise, (name, i)


def test_from_wavs_trains_a_model(ops):
    from drnmf_amd import layers
    rng = np.random.default_rng(9)
    clean = [(rng.standard_normal(n) * 2000 * (1 + np.sin(np.arange(n) / 300.0))).astype(np.int16)
             for n in (1200, 800, 1000, 640)]
    noisy = [(c + rng.standard_normal(len(c)) * 800).astype(np.int16) for c in clean]
    params = dict(cf="ed", sparsity=0.1, max_iter=8, conv_eps=0., random_seed=2016, r=100, n_iter=R.N_ITER)
    m = layers.SparseNMFModel.from_wavs(noisy, clean, params, N=N_M, hop=HOP_M, device=DEV)
    W = m.get_weights()[0]
    assert W.shape == (F_M, 200) and (m.r, m.n_iter, m.beta) == (100, R.N_ITER, 2.0)
    np.testing.assert_allclose((W.astype(np.float64) ** 2).sum(axis=0), 1.0, rtol=1e-4)
    xf, yf = ops.wavs_to_frames(noisy, clean, N_M, HOP_M)
    irm = m.forward(xf[None])[0]
    want = float(np.mean((irm.cpu().numpy().astype(np.float64) * xf.cpu().numpy() - yf.cpu().numpy()) ** 2))
    got = m.val_loss(noisy, clean, N=N_M, hop=HOP_M)
    print("snmf from_wavs: val_loss %.6e, by hand %.6e" % (got, want))
    assert np.isfinite(got) and got > 0 and abs(got - want) <= 1e-5 * want     # float32 mean against float64
    with pytest.raises(NotImplementedError, match="from_wavs"):
        m.compile()
