"""The device SDR (csrc/sdr.hip) stage by stage on the MI355X, at the shapes its kernels branch on: the tiled
correlation bitwise against integer sums, the Levinson solve by its residual against LU on the same system, the
projection against long double within a derived bound, the score against the mpmath solution, and the flags.
The references are in sdr_ref.py (checked on the CPU in test_sdr_ref_host.py); none of them is the code under test."""
import functools

import numpy as np
import pytest
import torch

import sdr_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLENS = [1, 7, 8, 9, 31, 511, 512, 513, 1000, 1024, 2047, 2048]
GRID_LENGTHS = [1, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 16385, 20011]
PROJ_OUT = 2048


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _lengths(flen):
    """The grid's row lengths, the lengths at which len + flen - 1 straddles a multiple of PROJ_OUT
    (len = 2048 k - flen + 1 + {-1, 0, 1}, k = 1, 2) and lengths below flen."""
    out = list(GRID_LENGTHS)
    for k in (1, 2):
        out += [PROJ_OUT * k - flen + 1 + e for e in (-1, 0, 1)]
    out += [1, flen // 2, flen - 1]
    return [n for n in out if n >= 1]


def _poisoned(nbytes):
    """A workspace of the test's own, every byte 0xFF: a double read from it before it was written is a NaN."""
    return torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device=DEV)


def _run(ops, E, X, lens, flen):
    """drnmf_sdr_ragged with every output and the workspace the test's own; lens a device int64 tensor or None.
    The workspace is poisoned, so a partial sum that is read without having been written (a split or a block
    beyond the row's own) turns the result into NaN whatever the allocator would have handed out."""
    from drnmf_amd import _capi
    n_sig = E.shape[0]
    ws = _poisoned(_capi.lib().drnmf_sdr_ragged_workspace_bytes(n_sig, E.shape[1], int(flen)))
    f64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
    out = dict(db=torch.full((n_sig,), float("nan"), dtype=torch.float32, device=DEV), coef=f64(n_sig, flen),
               en=f64(n_sig, 2), r=f64(n_sig, flen), d=f64(n_sig, flen),
               info=torch.full((n_sig,), -1, dtype=torch.int32, device=DEV))
    ops.sdr_ragged_enqueue(_t(E), _t(X), lens, flen, out["db"], coef=out["coef"], energies=out["en"], r=out["r"],
                           d=out["d"], info=out["info"], workspace=ws)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


_grid_cache = {}


def _grid(ops, flen):
    """One ragged batch per flen: int16-valued rows (estimate = the reference through a short filter plus
    noise), junk -- not zeros -- behind each row's length."""
    if flen in _grid_cache:
        return _grid_cache[flen]
    rng = np.random.default_rng(1000 + flen)
    lens = _lengths(flen)
    width = max(lens) + 13
    Ei = np.zeros((len(lens), width), np.int64)
    Xi = np.zeros((len(lens), width), np.int64)
    E = (3.0 * rng.standard_normal((len(lens), width))).astype(np.float32)
    X = (3.0 * rng.standard_normal((len(lens), width))).astype(np.float32)
    for i, n in enumerate(lens):
        x = rng.standard_normal(n + 8)
        x = np.convolve(x, [1.0, 0.6, 0.3])[:n + 8]               # mildly coloured
        y = np.convolve(x, [0.8, -0.4, 0.2, 0.1])[:n + 8] + 0.1 * rng.standard_normal(n + 8)
        xi, x32 = S.int16_values(x[8:] if np.any(x[8:]) else np.ones(n))
        yi, y32 = S.int16_values(y[8:] if np.any(y[8:]) else np.ones(n))
        Xi[i, :n], X[i, :n], Ei[i, :n], E[i, :n] = xi, x32, yi, y32
    got = _run(ops, E, X, _t(np.array(lens, np.int64)), flen)
    _grid_cache[flen] = (lens, E, X, Ei, Xi, got)
    return _grid_cache[flen]


@pytest.mark.parametrize("flen", FLENS)
def test_correlation_is_exact(ops, flen):
    """(a) r and d of every row and lag are bitwise exact_corr / 2^30: every partial sum is an integer below 2^53
    in units of 2^-30, so no order of fp64 operations can round (sdr_ref's docstring).  Tolerance zero."""
    lens, E, X, Ei, Xi, got = _grid(ops, flen)
    for i, n in enumerate(lens):
        r, d = S.exact_corr_f64(Ei[i, :n], Xi[i, :n], flen)
        bad_r, bad_d = np.flatnonzero(got["r"][i] != r), np.flatnonzero(got["d"][i] != d)
        assert bad_r.size == 0 and bad_d.size == 0, \
            "flen %d row %d len %d: r differs at lags %s, d at %s" % (flen, i, n, bad_r[:8], bad_d[:8])


@pytest.mark.parametrize("flen", [512, 513])
def test_host_solver_correlation_is_exact(ops, flen):
    """(a) the same on drnmf_sdr_corr (csrc/score.hip, the host-solver path): full rows."""
    from drnmf_amd import _capi
    rng = np.random.default_rng(77 + flen)
    n_sig, n = 3, 20011
    Ei = rng.integers(-S.PEAK, S.PEAK + 1, size=(n_sig, n))
    Xi = rng.integers(-S.PEAK, S.PEAK + 1, size=(n_sig, n))
    e, x = _t((Ei / S.SCALE).astype(np.float32)), _t((Xi / S.SCALE).astype(np.float32))
    L = _capi.lib()
    h = _capi.handle(0)
    r = torch.full((n_sig, flen), float("nan"), dtype=torch.float64, device=DEV)
    d = torch.full_like(r, float("nan"))
    ws = _poisoned(L.drnmf_sdr_workspace_bytes(n_sig, n, flen))
    rc = L.drnmf_sdr_corr(h, n_sig, n, flen, _capi.ptr(e), _capi.ptr(x), _capi.ptr(r), _capi.ptr(d), _capi.ptr(ws),
                          ws.numel(), ops._stream())
    _capi.check(rc, h, "drnmf_sdr_corr")
    r, d = r.cpu().numpy(), d.cpu().numpy()
    for i in range(n_sig):
        wr, wd = S.exact_corr_f64(Ei[i], Xi[i], flen)
        assert np.array_equal(r[i], wr) and np.array_equal(d[i], wd), (flen, i)


@pytest.mark.parametrize("flen", FLENS)
def test_projection_within_the_running_error_bound(ops, flen):
    """(c) with the device's own coefficients as INPUT, the two energies equal sdr_ref.project_ld's long double
    figures within sdr_ref.projection_bound, computed from the row's samples and coefficients (not a tuned
    constant).  Rows: the grid, lengths where len + flen - 1 straddles a multiple of 2048, and len < flen."""
    lens, E, X, Ei, Xi, got = _grid(ops, flen)
    assert np.all(np.isfinite(got["coef"])), "non-finite coefficients"
    worst = 0.0
    for i, n in enumerate(lens):
        num, den, Bn, Bd = S.project_ld(E[i, :n], X[i, :n], got["coef"][i])
        for name, have, want, B in (("num", got["en"][i, 0], num, Bn), ("den", got["en"][i, 1], den, Bd)):
            tol = S.projection_bound(n, flen, B)
            err = abs(float(np.longdouble(have) - want))
            worst = max(worst, err / tol if tol > 0 else (0.0 if err == 0 else np.inf))
            assert err <= tol, "flen %d row %d len %d %s: |%r - %r| = %.3e > bound %.3e" % (
                flen, i, n, name, have, float(want), err, tol)
    print("projection flen=%d: %d rows, worst error / bound = %.3e" % (flen, len(lens), worst))


# ---- the solve and the score on the badly conditioned families -------------------------------------------------

@functools.lru_cache(maxsize=None)
def _families_ints():
    import test_gpu_sdr as T
    E, X = T._families()
    return E, X, np.stack([S.as_int16_values(e) for e in E]), np.stack([S.as_int16_values(x) for x in X])


_family_cache = {}


def _family_run(ops, flen, rows):
    key = (flen, tuple(rows))
    if key not in _family_cache:
        E, X, Ei, Xi = _families_ints()
        E, X = E[list(rows)], X[list(rows)]
        got = _run(ops, E, X, None, flen)
        c_mp = [S.levinson_mp(got["r"][i], got["d"][i]) for i in range(len(rows))]
        _family_cache[key] = (E, X, got, c_mp)
    return _family_cache[key]


RESIDUAL_FACTOR = 10.0


def _check_solve(tag, r, d, c_dev, c_mp):
    c_lu = np.linalg.solve(S.toeplitz(r), d)
    res_dev, res_lu = S.scaled_residual(r, d, c_dev), S.scaled_residual(r, d, c_lu)
    cm = S.mp_to_f64(c_mp)
    fwd = lambda c: float(np.linalg.norm(c - cm) / np.linalg.norm(cm))
    print("%s: scaled residual device %.3e, LU %.3e, ratio %.2f; forward error device %.3e, LU %.3e" % (
        tag, res_dev, res_lu, res_dev / res_lu, fwd(c_dev), fwd(c_lu)))
    return res_dev, res_lu


@pytest.mark.parametrize("flen,rows", [(512, tuple(range(8))), (2048, (0,))])
def test_solve_residual_on_badly_conditioned_systems(ops, flen, rows):
    """(b) on the device's own r and d (eight families at flen = 512, condition numbers up to 1.9e9; family 0 at
    2048): info = 0, and the scaled residual ||T c - d||_inf / (||T||_inf ||c||_inf + ||d||_inf) of the device's
    c, evaluated exactly, is at most 10 times that of np.linalg.solve on the same system -- LU with pivoting is
    backward stable and sets the scale, the factor allows for Levinson being only weakly stable.  The forward
    errors against the mpmath solution are printed, not asserted: at these condition numbers neither solver owes
    a small one.

    Measured on the MI355X: residual ratios device / LU of 4.1, 1.5, 6.4, 6.5, 1.7, 0.8, 0.5, 3.1 on
    the eight families at flen = 512 and 1.5 on family 0 at 2048."""
    E, X, got, c_mp = _family_run(ops, flen, rows)
    assert np.all(got["info"] == 0), got["info"]
    failed = []
    for k, fam in enumerate(rows):
        res_dev, res_lu = _check_solve("solve flen=%d family %d" % (flen, fam), got["r"][k], got["d"][k],
                                       got["coef"][k], c_mp[k])
        if not res_dev <= RESIDUAL_FACTOR * res_lu:
            failed.append((fam, res_dev, res_lu))
    assert not failed, failed


# max over the eight families of |oracle.sdr_db - dB of project_ld at the mpmath solution|: 8.6e-13 dB as measured on
# the CPU.  The source of truth is test_sdr_ref_host.py::test_oracle_db_error_on_the_families, which recomputes it and
# asserts that four times the recomputed figure is within SCORE_TOL_DB; this constant is a record of that measurement.
# Four times it is below the floor, so the floor of 1e-9 dB is the tolerance.
ORACLE_VS_MP_DB = 8.6e-13
SCORE_TOL_DB = max(4.0 * ORACLE_VS_MP_DB, 1e-9)


def test_score_against_the_mpmath_solution(ops):
    """(d) the dB computed in fp64 from the device's energies against the dB of project_ld at the mpmath solution
    of the device's own system, within SCORE_TOL_DB (the oracle's own error sets the scale); and the float32
    sdr_out within one float32 ulp of float32(10 log10(en0 / en1)) of the device's own energies."""
    rows = tuple(range(8))
    E, X, got, c_mp = _family_run(ops, 512, rows)
    worst = 0.0
    for k in rows:
        num, den, _, _ = S.project_ld(E[k], X[k], S.mp_to_ld(c_mp[k]))
        want = S.db(num, den)
        have = 10.0 * np.log10(got["en"][k, 0] / got["en"][k, 1])
        worst = max(worst, abs(have - want))
        print("score family %d: device %.12f mp %.12f diff %.3e dB" % (k, have, want, have - want))
        f32 = np.float32(have)
        assert abs(np.float32(got["db"][k]) - f32) <= np.spacing(f32), (k, got["db"][k], f32)
    print("score: max |device - mp| = %.3e dB (tolerance %.1e)" % (worst, SCORE_TOL_DB))
    assert worst <= SCORE_TOL_DB, worst


# ---- flags and clamping ------------------------------------------------------------------------------------------

def test_early_stop_beyond_one_pair_per_lane(ops):
    """(e) r = the autocorrelation of 65 real sinusoids (rank 130), n = 300: the prediction error collapses near
    step 130, where a lane owns more than one index pair.  info >= 2, c is zero from info - 2 on, and c[:info - 2]
    solves the leading system of that order with a residual within 10 times LU's.  The step is not asserted."""
    n = 300
    rng = np.random.default_rng(0)
    w = np.pi * (np.arange(65) + 0.5 + 0.3 * rng.uniform(-1, 1, 65)) / 65
    A = rng.uniform(0.7, 1.3, 65)
    r = (A[None] ** 2 / 2 * np.cos(w[None] * np.arange(n)[:, None])).sum(1)
    d = rng.standard_normal(n) * r[0]
    c, info = ops.toeplitz_solve(_t(r), _t(d))
    c, info = c.cpu().numpy(), int(info.cpu().numpy()[0])
    print("early stop: info = %d (step %d)" % (info, info - 2))
    assert info >= 2, info
    k = info - 2
    assert 128 <= k < n, k                  # (k + 1) >> 1 > 64: a lane has owned more than one pair; not the exact step
    assert np.all(c[k:] == 0.0) and np.all(np.isfinite(c))
    c_lu = np.linalg.solve(S.toeplitz(r[:k]), d[:k])
    res_dev, res_lu = S.scaled_residual(r, d, c[:k]), S.scaled_residual(r, d, c_lu)
    print("early stop: scaled residual of the order-%d solution: device %.3e, LU %.3e" % (k, res_dev, res_lu))
    assert res_dev <= RESIDUAL_FACTOR * res_lu, (res_dev, res_lu)


def test_device_lengths_are_clamped(ops):
    """(e) device-tensor lengths of -5 and width + 9 give the bits of lengths 0 and width, and the rows next to
    them keep theirs."""
    flen, width = 64, 3000
    rng = np.random.default_rng(5)
    Xi = rng.integers(-S.PEAK, S.PEAK + 1, size=(5, width))
    Ei = np.round(0.7 * Xi + 0.2 * np.roll(Xi, 3, axis=1) + 500 * rng.standard_normal((5, width))).astype(np.int64)
    E, X = (Ei / S.SCALE).astype(np.float32), (Xi / S.SCALE).astype(np.float32)
    wild = _run(ops, E, X, _t(np.array([1500, -5, 2999, width + 9, 17], np.int64)), flen)
    tame = _run(ops, E, X, _t(np.array([1500, 0, 2999, width, 17], np.int64)), flen)
    for key in ("db", "coef", "en", "r", "d", "info"):
        assert wild[key].tobytes() == tame[key].tobytes(), key
    assert wild["info"].tolist() == [0, 1, 0, 0, 0]
    assert np.all(wild["r"][1] == 0.0) and np.all(wild["coef"][1] == 0.0)
    r3, d3 = S.exact_corr_f64(Ei[3], Xi[3], flen)
    assert np.array_equal(wild["r"][3], r3) and np.array_equal(wild["d"][3], d3)
