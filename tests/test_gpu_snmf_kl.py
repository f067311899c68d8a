"""The sparse-NMF baseline under the KL cost on the MI355X (csrc/snmf_kl.hip, include/drnmf_snmf_kl.h,
layers.SparseNMFModel with beta = 1): the one-launch kernel against the fp64 reference of tests/snmf_kl_ref.py
(oracle.mu_infer at beta = 1 + oracle.snmf_irm per valid frame, one shared initial vector), with and without zero bins
and under both rules for the floor, its bitwise independence of a row from its position and its neighbours, its
distance from the GEMM path at beta = 1, and the model surface (routing, predict, stream, enhance).

Cases (B, T, F, N), 30 iterations, sparsity 0.1: the four of tests/test_gpu_snmf_model.py plus
  (1, 2, 40, 256)    the widest shape of the narrow instance (np16(N) = 256)
  (1, 3, 33, 258)    the first shape of the wide instance, with scalar dictionary loads (N % 4 != 0)
The entry exposes the mask only (H stays on chip), so the bound is the project's mask bound, MASK_MSE_TOL; the float32
restatement of tests/test_snmf_kl_host.py sits five orders below it."""
import numpy as np
import pytest
import torch

import snmf_kl_ref as K
import snmf_model_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_M, HOP_M, F_M = 256, 64, 129          # the model-level tests: a small model, N = 200 atoms
LIVE = (3, 7, 129, 200)


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _dev(*arrays):
    return tuple(torch.from_numpy(np.array(a, copy=True)).to(DEV) for a in arrays)


def _run(ops, case, zeros=False, v_floor=None, power=1.0, n_iter=R.N_ITER):
    x, W, h_init = K.zero_problem(*case) if zeros else R.problem(*case)
    Wn, hn = R.normalised(W, h_init)
    xd, Wd, hd = _dev(x, Wn, hn)
    out = ops.snmf_kl_forward(xd, Wd, hd, R.SPARSITY, n_iter, power=power, mask_value=R.MASK_VALUE, v_floor=v_floor)
    return out.cpu().numpy()


def _check(got, case, what, **ref_kw):
    ref = K.case_reference(*case, **ref_kw)
    valid = R.valid_frames(case[0], case[1])
    mse = float(np.mean((got - ref) ** 2))
    print("snmf kl mask %s %s: MSE %.3e, max |d| %.3e" % (case, what, mse, float(np.max(np.abs(got - ref)))))
    assert np.isfinite(got).all()
    assert not got[~valid].any(), "masked rows must be exactly 0"
    assert mse <= R.MASK_MSE_TOL, (case, what, mse)


@pytest.mark.parametrize("case", K.CASES)
def test_mask_against_the_reference(ops, case):
    _check(_run(ops, case), case, "kl")


@pytest.mark.parametrize("v_floor", [None, K.V_FLOOR])
@pytest.mark.parametrize("case", R.CASES)
def test_zero_bins_against_the_reference(ops, case, v_floor):
    """v_floor=None: the oracle's own rule (zeros raised to the smallest positive entry of the frames run together);
    v_floor=1e-3: the oracle on the input with its zeros replaced by the constant."""
    got = _run(ops, case, zeros=True, v_floor=v_floor)
    _check(got, case, "zero bins, v_floor=%s" % v_floor, zeros=True, v_floor=v_floor)
    if case == LIVE:                      # the frame that is zero in every bin is a constant frame: a mask like any
        b, t = K.ZERO_FRAME[(3, 7)]
        assert got[b, t].std() > 0.05


def test_the_pre_pass_is_the_definition_of_the_floor(ops):
    """Bitwise: v_floor=None equals v_floor = the smallest positive V of the valid rows, computed with torch."""
    for case, power in ((LIVE, 1.0), ((1, 17, 33, 48), 1.0), (LIVE, 2.0)):
        x = K.zero_problem(*case)[0]
        xv = torch.from_numpy(x[K.valid_of(x)].copy()).to(DEV)
        floor = float(xv[xv > 0].min() ** power)
        a = _run(ops, case, zeros=True, v_floor=None, power=power)
        b = _run(ops, case, zeros=True, v_floor=floor, power=power)
        assert np.array_equal(a, b), (case, power)
        c = _run(ops, case, zeros=True, v_floor=floor * 1.5, power=power)      # ... and the floor is live
        assert not np.array_equal(a, c)


def test_no_positive_entry(ops):
    """A call whose valid frames are all zero: the floor is 0, nothing is raised, the masks are 0 and finite."""
    _, W, h_init = R.problem(*LIVE)
    Wn, hn = R.normalised(W, h_init)
    x = np.zeros((1, 5, 129), np.float32)
    x[0, 3] = R.MASK_VALUE
    xd, Wd, hd = _dev(x, Wn, hn)
    got = ops.snmf_kl_forward(xd, Wd, hd, R.SPARSITY, R.N_ITER, mask_value=R.MASK_VALUE).cpu().numpy()
    assert np.isfinite(got).all() and not got.any()


def test_spectrogram_power_two(ops):
    _check(_run(ops, LIVE, power=2.0), LIVE, "power 2", power=2.0)
    _check(_run(ops, LIVE, zeros=True, power=2.0), LIVE, "power 2, zero bins", zeros=True, power=2.0)


def test_general_spectrogram_power(ops):
    """A power other than 1 and 2 runs instances of its own (powf in the chunk loop)."""
    _check(_run(ops, LIVE, zeros=True, power=1.5), LIVE, "power 1.5, zero bins", zeros=True, power=1.5)
    case = (2, 9, 257, 512)
    _check(_run(ops, case, power=0.5), case, "power 0.5", power=0.5)


@pytest.mark.parametrize("zeros,v_floor", [(True, K.V_FLOOR), (False, None)])
def test_rows_do_not_depend_on_position_or_neighbours(ops, zeros, v_floor):
    """Bitwise: the mask of (3, 7, 129, 200) equals the masks of the same rows run one sequence at a time, one frame
    at a time and seven positions further on -- with zero bins under a fixed floor, and without zero bins under the
    reference's rule, where the floor is never used."""
    x, W, h_init = K.zero_problem(*LIVE) if zeros else R.problem(*LIVE)
    Wn, hn = R.normalised(W, h_init)
    xd, Wd, hd = _dev(x, Wn, hn)
    ws = torch.empty(256, dtype=torch.uint8, device=DEV)
    run = lambda v: ops.snmf_kl_forward(v.contiguous(), Wd, hd, R.SPARSITY, R.N_ITER, mask_value=R.MASK_VALUE,
                                        v_floor=v_floor, workspace=ws)
    whole = run(xd)
    by_seq = torch.cat([run(xd[b:b + 1]) for b in range(LIVE[0])])
    by_frame = torch.cat([torch.cat([run(xd[b:b + 1, t:t + 1]) for t in range(LIVE[1])], dim=1)
                          for b in range(LIVE[0])])
    assert torch.equal(whole, by_seq)
    assert torch.equal(whole, by_frame)
    shifted = run(torch.cat([xd[2:], xd[:2]]))                    # the same rows 7 positions further on
    assert torch.equal(whole, torch.cat([shifted[1:], shifted[:1]]))
    assert float(whole.std()) > 0.05


@pytest.mark.parametrize("case", [LIVE, (2, 9, 257, 512)])
def test_against_the_gemm_path(ops, case):
    """Max abs difference from ops.snmf_mask_forward(beta=1, path='gemm') within 1e-5, the project's bound between its
    two paths (tests/test_gpu_snmf_model.py); measured values: DESIGN.md section 6h."""
    for zeros in (False, True):
        x, W, h_init = K.zero_problem(*case) if zeros else R.problem(*case)
        Wn, hn = R.normalised(W, h_init)
        xd, Wd, hd = _dev(x, Wn, hn)
        kl = ops.snmf_kl_forward(xd, Wd, hd, R.SPARSITY, R.N_ITER, mask_value=R.MASK_VALUE)
        gemm = ops.snmf_mask_forward(xd, Wd, hd, R.SPARSITY, R.N_ITER, beta=1.0, mask_value=R.MASK_VALUE, path="gemm")
        d = float((kl - gemm).abs().max())
        print("snmf kl %s zeros=%s: max |kl kernel - gemm path| %.3e" % (case, zeros, d))
        assert d <= 1e-5, (case, zeros, d)


def test_no_iteration_is_the_mask_of_h_init(ops):
    for case in (LIVE, (1, 3, 33, 258)):
        x, W, h_init = R.problem(*case)
        Wn, hn = R.normalised(W, h_init)
        r = case[3] // 2
        c = Wn[:, :r].astype(np.float64) @ hn[:r].astype(np.float64)
        n = Wn[:, r:].astype(np.float64) @ hn[r:].astype(np.float64)
        want = np.where(R.valid_frames(case[0], case[1])[..., None], (c / (1e-9 + c + n))[None, None, :], 0.0)
        got = _run(ops, case, n_iter=0)
        assert float(np.max(np.abs(got - want))) <= 1e-6 and not got[~R.valid_frames(case[0], case[1])].any()
        _check(got, case, "0 iterations", n_iter=0)


# ---- the model ---------------------------------------------------------------------------------------------------
def _model(n_iter=R.N_ITER, **kw):
    from drnmf_amd import layers
    _, W, h_init = R.problem(3, 7, F_M, 200)
    return layers.SparseNMFModel(W, 100, R.SPARSITY, n_iter=n_iter, beta=1.0, h_init=h_init, device=DEV, **kw)


def _recordings(silence=True):
    """Three recordings; silence: with stretches of digital silence -- whole frames of zero bins inside valid audio."""
    rng = np.random.default_rng(5)
    wavs = [(rng.standard_normal(n) * 3000 * (1 + 0.5 * np.sin(np.arange(n) / 700.0))).astype(np.int16)
            for n in (1500, 2317, 900)]
    if silence:
        wavs[0][300:900] = 0
        wavs[1][:700] = 0
        wavs[2][500:] = 0
    return wavs


def test_default_iteration_count_against_the_reference(ops):
    """n_iter = 200, the reference's inference setting (enhance.py:842), through model.forward."""
    from drnmf_amd import layers
    x, W, h_init = R.problem(*LIVE)
    m = layers.SparseNMFModel(W, 100, R.SPARSITY, beta=1.0, h_init=h_init, path="tile", device=DEV)
    assert m.n_iter == 200
    got = m.forward(torch.from_numpy(x.copy()).to(DEV)).cpu().numpy()
    _check(got, LIVE, "200 iterations", n_iter=200)


def test_model_paths_are_the_ops_they_name(ops):
    x, W, h_init = K.zero_problem(*LIVE)
    Wn, hn = R.normalised(W, h_init)
    xd = torch.from_numpy(x.copy()).to(DEV)
    tile, gemm, fixed = _model(path="tile"), _model(path="gemm"), _model(v_floor=K.V_FLOOR)
    Wd, hd = tile._operands()
    np.testing.assert_allclose(Wd.cpu().numpy(), Wn, rtol=1e-6)
    kw = dict(mask_value=R.MASK_VALUE)
    assert torch.equal(tile.forward(xd), ops.snmf_kl_forward(xd, Wd, hd, R.SPARSITY, R.N_ITER, **kw))
    assert torch.equal(gemm.forward(xd), ops.snmf_mask_forward(xd, Wd, hd, R.SPARSITY, R.N_ITER, beta=1.0,
                                                               path="gemm", **kw))
    assert torch.equal(fixed.forward(xd), ops.snmf_kl_forward(xd, Wd, hd, R.SPARSITY, R.N_ITER, v_floor=K.V_FLOOR,
                                                              **kw))
    assert not torch.equal(fixed.forward(xd), tile.forward(xd))


def _small(rows, **kw):
    """The 5 x 10 dictionary of test_gpu_snmf_model.test_auto_rule_follows_the_row_count: (model, x [1, rows, 5])."""
    from drnmf_amd import layers
    _, W, h_init = R.problem(1, 1, 5, 10)
    x = torch.rand((1, rows, 5), generator=torch.Generator().manual_seed(1)).to(DEV) + 0.01
    mk = lambda **k: layers.SparseNMFModel(W, 5, R.SPARSITY, n_iter=5, beta=1.0, h_init=h_init, device=DEV, **k)
    return mk, x


def test_auto_rule_follows_the_measured_row_count(ops):
    """path='auto' at beta = 1 is the KL kernel up to _capi.SNMF_KL_AUTO_MAX_ROWS rows and the GEMM path beyond: the
    same bits as the path it names."""
    from drnmf_amd import _capi
    rows = _capi.SNMF_KL_AUTO_MAX_ROWS
    if rows == 0:
        pytest.skip("SNMF_KL_AUTO_MAX_ROWS is 0: the KL kernel measured faster at no row count, 'auto' never takes it")
    mk, x = _small(rows + 1)
    auto, tile, gemm = mk(), mk(path="tile"), mk(path="gemm")
    assert torch.equal(auto.forward(x), gemm.forward(x))
    below = x[:, :rows].contiguous()
    assert torch.equal(auto.forward(below), tile.forward(below))


def test_a_fixed_floor_always_takes_the_kernel(ops):
    """With v_floor set, 'auto' above the measured row count is still the KL kernel."""
    from drnmf_amd import _capi
    mk, x = _small(_capi.SNMF_KL_AUTO_MAX_ROWS + 2)      # (two rows at least: the second holds no zero)
    x[0, 0, 2] = 0.0
    Wd, hd = mk()._operands()
    want = ops.snmf_kl_forward(x, Wd, hd, R.SPARSITY, 5, mask_value=R.MASK_VALUE, v_floor=K.V_FLOOR)
    assert torch.equal(mk(v_floor=K.V_FLOOR).forward(x), want)
    gemm = mk(path="gemm").forward(x)
    assert float((want - gemm).abs().max()) > 0 and float((want[:, 1:] - gemm[:, 1:]).abs().max()) <= 1e-5


def test_predict_in_slabs_equals_forward_row_by_row(ops):
    """Bitwise, on sequences that hold zero bins: with a fixed floor a frame is a function of that frame alone."""
    m = _model(v_floor=K.V_FLOOR)
    p = K.zero_problem(3, 7, F_M, 200)[0]
    x = np.stack([p[0], p[1], p[2], p[0][::-1], p[1]]).copy()      # 5 sequences: ragged, one all masked
    x[4, :3] = R.MASK_VALUE                                        # ... and one that starts masked
    got = m.predict(x, batch_size=2)
    rows = np.concatenate([m.forward(torch.from_numpy(x[i:i + 1]).to(DEV)).cpu().numpy() for i in range(5)])
    assert np.array_equal(got, rows)
    assert np.array_equal(m.predict_on_batch(x), rows)
    masked = ~np.any(x != R.MASK_VALUE, axis=-1)
    assert masked.any() and not got[masked].any() and got[~masked].std() > 0.05
    assert (x[~masked] == 0).any()


def test_stream_equals_the_whole_recording(ops):
    """model.stream over uneven chunks (empty ones included) of recordings with digital silence, against `enhance` on
    the whole recordings: bitwise under a fixed floor."""
    from test_gpu_stream import _model_schedules, _push_all
    m = _model(v_floor=K.V_FLOOR)
    wavs = _recordings()
    lens = [len(w) for w in wavs]
    rf, masks = m.enhance(wavs, N=N_M, hop=HOP_M, dtype="float32", crop=True, return_masks=True)
    pcm = np.zeros((len(wavs), max(lens)), np.int16)
    for i, w in enumerate(wavs):
        pcm[i, :len(w)] = w
    x, _, _, nf = ops.stft_ragged(torch.from_numpy(pcm).to(DEV), lens, N=N_M, hop=HOP_M, mask_value=R.MASK_VALUE)
    silent = [(x[i, :int(nf[i])] == 0).all(dim=-1) for i in range(len(wavs))]
    assert all(bool(s.any()) and not bool(s.all()) for s in silent)          # zero frames inside valid audio
    for name, sch in _model_schedules(wavs).items():
        yf = _push_all(m.stream(len(wavs), N=N_M, hop=HOP_M, dtype="float32", crop=True), wavs, sch)
        for i, n in enumerate(lens):
            assert yf[i].shape == (n,)
            assert np.array_equal(yf[i], rf[i]), (name, i)
    assert all(np.isfinite(k).all() for k in masks)


def test_enhance_scores(ops):
    m = _model(v_floor=K.V_FLOOR)
    wavs = _recordings(silence=False)
    clean = [(0.8 * w).astype(np.int16) for w in wavs]
    out, S, labels = m.enhance(wavs, N=N_M, hop=HOP_M, ref=clean)
    assert len(out) == 3 and out[0].dtype == np.int16
    assert np.asarray(S).shape == (3, 6) and len(labels) == 6
