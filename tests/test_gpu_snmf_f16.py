"""The sparse-NMF baseline on fp16 matrix-core operands on the MI355X (csrc/snmf_f16.hip, include/drnmf_snmf_f16.h,
SparseNMFModel(operand_dtype='float16')): the kernel against the fp64 emulation of tests/snmf_f16_ref.py (which rounds
the operands the kernel rounds) and against the fp64 oracle (oracle.mu_infer + oracle.snmf_irm), its range, the
bitwise independence of a row from its position and neighbours, and the inherited model surface.

Cases (B, T, F, N), 30 iterations, sparsity 0.1 (snmf_f16_ref.CASES, masked rows in every case that has room):
  (1, 1, 5, 10)      one row in a padded tile, one partial chunk, N < 16
  (1, 17, 33, 48)    two row tiles, the second one masked entirely; F = 32 + 1; three column tiles over four waves
  (3, 7, 129, 200)   the shipped N, 21 rows, ragged lengths and one all-masked sequence
  (1, 3, 40, 258)    the first shape of the wide instance (17 column tiles)
  (2, 9, 257, 512)   the widest shape, masked frames in the interior
and spectrogram_power = 2 and 200 iterations at (3, 7, 129, 200).

Bounds (snmf_f16_ref.TOL_EMU, TOL_EXACT).  Masks lie in [0, 1]: absolute, max over elements.  Measured on the MI355X,
device - emulation / device - fp64 oracle:
  (1, 1, 5, 10) 3.4e-7 / 6.0e-4    (1, 17, 33, 48) 6.5e-5 / 1.0e-3    (3, 7, 129, 200) 9.3e-6 / 1.6e-4
  (1, 3, 40, 258) 9.1e-6 / 1.5e-4  (2, 9, 257, 512) 5.5e-6 / 3.7e-5   power 2 2.3e-5 / 2.1e-4
  200 iterations 1.7e-5 / 1.2e-3   range tile 9.8e-6 / 1.6e-4 (rows: ordinary 2.4e-6 / 1.1e-4, x 1e-6 4e-103 both, x 1e4
  9.8e-6 / 1.0e-4, all zero 0 / 0, single zero bins 6.8e-6 / 9.9e-5, x 1e-16 and x 1e-30 0 / 0)
  (3, 7, 129, 200) x 2^-20 9.3e-6 / 1.6e-4, x 2^14 9.3e-6 / 1.6e-4 (sparsity and h_init scaled along)
  worst device - emulation 6.489e-5 -> TOL_EMU   = 4 x = 2.60e-4
  worst device - oracle    1.162e-3 -> TOL_EXACT = 4 x = 4.65e-3
Device and emulation can leave an H or a Lambda on different sides of an fp16 rounding boundary -- the device sums in
fp32, the emulation in fp64 -- so TOL_EMU is far above fp32 noise.  The distance to the oracle is that of the emulation
itself (test_snmf_f16_host.py prints it per case): it is what the fp16 operands cost, not a property of the kernel."""
import numpy as np
import pytest
import torch

import snmf_f16_ref as E
import snmf_model_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL_EMU, TOL_EXACT = E.TOL_EMU, E.TOL_EXACT
N_M, HOP_M, F_M = 256, 64, 129          # the model-level tests: a small model, N = 200 atoms


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _forward(ops, x, W, h_init, n_iter=R.N_ITER, power=1.0):
    Wn, hn = R.normalised(W, h_init)
    t = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    Wd = t(Wn)
    return ops.snmf_f16_forward(t(x), ops.snmf_f16_pack_dict(Wd), Wd, t(hn), R.SPARSITY, n_iter, power=power,
                                mask_value=R.MASK_VALUE)


def _check(got, emu, ref, masked, what):
    d_emu, d_exact = float(np.max(np.abs(got - emu))), float(np.max(np.abs(got - ref)))
    print("snmf f16 %s: max |device - emulation| %.3e, max |device - oracle| %.3e" % (what, d_emu, d_exact))
    assert np.isfinite(got).all()
    assert not got[masked].any(), "masked rows must be exactly 0"
    assert got.min() >= 0 and got.max() <= 1
    assert d_emu <= TOL_EMU, (what, d_emu)
    assert d_exact <= TOL_EXACT, (what, d_exact)


@pytest.mark.parametrize("case", E.CASES)
def test_mask_against_the_emulation_and_the_oracle(ops, case):
    x, W, h_init = E.problem(*case)
    got = _forward(ops, x, W, h_init).cpu().numpy()
    _check(got, E.case_emulation(*case), E.case_reference(*case), ~E.valid_frames(*case), str(case))
    assert got[E.valid_frames(*case)].std() > 0.05


def test_packed_dictionary(ops):
    """float16 [F][N rounded up to 32], round to nearest even, zero behind N."""
    _, W, h_init = E.problem(1, 3, 40, 258)
    Wn, _ = R.normalised(W, h_init)
    d16 = ops.snmf_f16_pack_dict(torch.from_numpy(Wn.copy()).to(DEV)).cpu().numpy()
    assert d16.shape == (40, 288) and d16.dtype == np.float16
    assert np.array_equal(d16[:, :258], Wn.astype(np.float16)) and not d16[:, 258:].any()


def test_spectrogram_power_two(ops):
    case = E.LIVE
    x, W, h_init = E.problem(*case)
    got = _forward(ops, x, W, h_init, power=2.0).cpu().numpy()
    _check(got, E.case_emulation(*case, power=2.0), E.case_reference(*case, power=2.0), ~E.valid_frames(*case),
           "%s power 2" % (case,))


def test_default_iteration_count(ops):
    """n_iter = 200, the reference's inference setting (enhance.py:842), through the model."""
    from drnmf_amd import layers
    case = E.LIVE
    x, W, h_init = E.problem(*case)
    m = layers.SparseNMFModel(W, 100, R.SPARSITY, h_init=h_init, operand_dtype="float16", device=DEV)
    assert m.n_iter == 200
    got = m.forward(torch.from_numpy(x.copy()).to(DEV)).cpu().numpy()
    _check(got, E.case_emulation(*case, n_iter=200), E.case_reference(*case, n_iter=200), ~E.valid_frames(*case),
           "%s 200 iterations" % (case,))


def test_range_of_one_tile(ops):
    """One tile of (.., 129, 200) holding an ordinary row, the same row x 1e-6 and x 1e4, an all-zero row that is
    not masked, a row with single zero bins, a masked row, and the row x 1e-16 and x 1e-30 -- so quiet that the
    scale's exponent is clamped and the scaled floor is at its largest (snmf_f16_ref.range_problem): everything
    finite, and every row within the bounds the ordinary row meets."""
    x, W, h_init = E.range_problem()
    got = _forward(ops, x, W, h_init).cpu().numpy()
    emu, ref = E.range_references()
    assert np.isfinite(got).all()
    for i, name in enumerate(E.RANGE_ROWS):
        d_emu, d_exact = float(np.max(np.abs(got[0, i] - emu[0, i]))), float(np.max(np.abs(got[0, i] - ref[0, i])))
        print("snmf f16 range row %d (%s): device - emulation %.3e, device - oracle %.3e" % (i, name, d_emu, d_exact))
    masked = np.zeros((1, 16), bool)
    masked[0, 5] = True
    _check(got, emu, ref, masked, "range tile")
    assert not got[0, 3].any()                                     # V = 0: H = 0, mask 0 / 1e-9


@pytest.mark.parametrize("k", E.SCALED_K)
def test_scaled_problems(ops, k):
    """The live problem times 2^k, sparsity and h_init scaled along so that H stays alive (snmf_f16_ref.scaled_problem):
    at 2^-20 Lambda would sit in fp16's subnormals without the per-row scale, at 2^14 it would overflow
    (test_snmf_f16_host.py shows that the emulation without the scale misses TOL_EXACT on both)."""
    x, W, h_init, sparsity = E.scaled_problem(k)
    Wn, hn = R.normalised(W, h_init)
    t = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    Wd = t(Wn)
    got = ops.snmf_f16_forward(t(x), ops.snmf_f16_pack_dict(Wd), Wd, t(hn), sparsity, R.N_ITER,
                               mask_value=R.MASK_VALUE).cpu().numpy()
    emu, ref = E.scaled_references(k)
    _check(got, emu, ref, ~E.valid_frames(*E.LIVE), "%s x 2^%d" % (E.LIVE, k))
    assert got[E.valid_frames(*E.LIVE)].std() > 0.05


def test_the_flag_is_live(ops):
    """The float32 model's mask on the live case is NOT within TOL_EMU of the emulation (it is the oracle's, up to
    fp32 noise), the float16 model's is: the emulation tells the two apart."""
    from drnmf_amd import layers
    x, W, h_init = E.problem(*E.LIVE)
    emu = E.case_emulation(*E.LIVE, n_iter=E.LIVE_ITER)
    xd = torch.from_numpy(x.copy()).to(DEV)
    d = {}
    for dt in ("float32", "float16"):
        m = layers.SparseNMFModel(W, 100, R.SPARSITY, n_iter=E.LIVE_ITER, h_init=h_init, path="tile", operand_dtype=dt,
                                  device=DEV)
        d[dt] = float(np.max(np.abs(m.forward(xd).cpu().numpy() - emu)))
    print("snmf f16 live case %s, %d iterations: float32 model - emulation %.3e, float16 model - emulation %.3e" %
          (E.LIVE, E.LIVE_ITER, d["float32"], d["float16"]))
    assert d["float16"] <= TOL_EMU < d["float32"]


def test_rows_do_not_depend_on_position_or_neighbours(ops):
    """Bitwise: the mask of (3, 7, 129, 200) equals the masks of the same rows run one sequence at a time, one frame
    at a time and shifted by a sequence."""
    case = (3, 7, 129, 200)
    x, W, h_init = E.problem(*case)
    Wn, hn = R.normalised(W, h_init)
    xd, Wd, hd = (torch.from_numpy(a.copy()).to(DEV) for a in (x, Wn, hn))
    d16 = ops.snmf_f16_pack_dict(Wd)
    run = lambda v: ops.snmf_f16_forward(v.contiguous(), d16, Wd, hd, R.SPARSITY, R.N_ITER, mask_value=R.MASK_VALUE)
    whole = run(xd)
    by_seq = torch.cat([run(xd[b:b + 1]) for b in range(case[0])])
    by_frame = torch.cat([torch.cat([run(xd[b:b + 1, t:t + 1]) for t in range(case[1])], dim=1)
                          for b in range(case[0])])
    assert torch.equal(whole, by_seq)
    assert torch.equal(whole, by_frame)
    shifted = run(torch.cat([xd[2:], xd[:2]]))                    # the same rows 7 positions further on
    assert torch.equal(whole, torch.cat([shifted[1:], shifted[:1]]))
    assert float(whole.std()) > 0.05


@pytest.mark.parametrize("case", E.CASES + ["range"])
def test_without_iterations_the_two_tile_kernels_agree_bitwise(ops, case):
    """n_iter = 0: both tile kernels compute the mask from h_init through nothing but the phases of csrc/snmf_tile.h
    (validity, the final-mask loop with its staging, partial sums and store).  The fp16 kernel's row scale is a power
    of two on H and on the epsilon, which commutes with every fp32 rounding of that chain while nothing leaves the
    normal range -- and these inputs do not (row scales from 2^-14 up to the clamp at 2^40 in the range problem)."""
    x, W, h_init = E.range_problem() if case == "range" else E.problem(*case)
    Wn, hn = R.normalised(W, h_init)
    xd, Wd, hd = (torch.from_numpy(np.array(a)).to(DEV) for a in (x, Wn, hn))
    f16 = ops.snmf_f16_forward(xd, ops.snmf_f16_pack_dict(Wd), Wd, hd, R.SPARSITY, 0, mask_value=R.MASK_VALUE)
    f32 = ops.snmf_mask_forward(xd, Wd, hd, R.SPARSITY, 0, mask_value=R.MASK_VALUE, path="tile")
    assert torch.equal(f16, f32)
    assert float(f32.max()) > 0


# ---- the model ---------------------------------------------------------------------------------------------------
def _model(n_iter=R.N_ITER):
    from drnmf_amd import layers
    _, W, h_init = R.problem(3, 7, F_M, 200)
    return layers.build_snmf(dict(r=100, sparsity=R.SPARSITY, cf="ed", n_iter=n_iter, operand_dtype="float16"), W,
                             device=DEV)


def _recordings():
    rng = np.random.default_rng(5)
    return [(rng.standard_normal(n) * 3000 * (1 + 0.5 * np.sin(np.arange(n) / 700.0))).astype(np.int16)
            for n in (1500, 2317, 900)]


def test_predict_in_slabs_equals_forward(ops):
    m = _model()
    assert m.operand_dtype == "float16"
    p = R.problem(3, 7, F_M, 200)[0]
    x = np.stack([p[0], p[1], p[2], p[0][::-1], p[1]]).copy()      # 5 sequences: ragged, one all masked
    x[4, :3] = R.MASK_VALUE                                        # ... and one that starts masked
    want = m.forward(torch.from_numpy(x).to(DEV))
    got = m.predict(x, batch_size=2)
    assert torch.equal(torch.from_numpy(got).to(DEV), want)        # bitwise: frames are independent
    assert np.array_equal(m.predict_on_batch(x), got)
    masked = ~np.any(x != R.MASK_VALUE, axis=-1)
    assert masked.any() and not got[masked].any() and got[~masked].std() > 0.05
    # the packed dictionary is kept with Wn and remade when W changes
    d16 = m._dict16()
    assert m._dict16() is d16 and d16.dtype == torch.float16 and tuple(d16.shape) == (F_M, 224)
    W = m.get_weights()[0]
    assert W.dtype == np.float32
    m.set_weights([W[:, ::-1].copy()])
    assert m._dict16() is not d16
    assert np.array_equal(m._dict16().cpu().numpy()[:, :200], m._operands()[0].cpu().numpy().astype(np.float16))


def test_stream_equals_the_whole_recording(ops):
    """model.stream in float32 over ragged cuts with empty chunks against the whole-recording enhance: bitwise."""
    from test_gpu_stream import _model_schedules, _push_all
    m = _model()
    wavs = _recordings()
    clean = [(0.8 * w).astype(np.int16) for w in wavs]
    rf = m.enhance(wavs, N=N_M, hop=HOP_M, dtype="float32", crop=True)
    yf = _push_all(m.stream(len(wavs), N=N_M, hop=HOP_M, dtype="float32", crop=True), wavs,
                   _model_schedules(wavs)["ragged"])
    for i, w in enumerate(wavs):
        assert yf[i].shape == (len(w),) and np.abs(rf[i]).max() > 0
        assert np.array_equal(yf[i], rf[i]), i
    out, S, labels = m.enhance(wavs, N=N_M, hop=HOP_M, ref=clean)
    assert len(out) == 3 and out[0].dtype == np.int16 and np.asarray(S).shape == (3, 6) and len(labels) == 6
