"""The references of sdr_ref.py checked on the CPU, each against something other than itself: exact_corr against the
oracle's FFT correlation, levinson_mp by its residual in mpmath, scaled_residual and project_ld against direct
evaluations, and the oracle-vs-mpmath dB error that sets the score tolerance of test_gpu_sdr_stages.py."""
import mpmath
import numpy as np
import pytest

import sdr_ref as S
from oracle import drnmf_oracle as O


def _pair(rng, n):
    x = np.convolve(rng.standard_normal(n), [1.0, 0.7, 0.2])[:n]
    y = np.convolve(x, [0.8, -0.3, 0.1])[:n] + 0.1 * rng.standard_normal(n)
    return S.int16_values(y), S.int16_values(x)


@pytest.mark.parametrize("n,flen", [(1, 1), (5, 9), (300, 7), (4097, 513), (20011, 2048)])
def test_exact_corr_against_the_fft_correlation(n, flen):
    rng = np.random.default_rng(n + flen)
    (yi, y32), (xi, x32) = _pair(rng, n)
    r, d = S.exact_corr_f64(yi, xi, flen)
    wr, wd = O.sdr_corr(y32, x32, flen)
    scale = max(np.max(np.abs(r)), np.max(np.abs(d)))
    assert np.max(np.abs(r - wr)) <= 1e-9 * scale and np.max(np.abs(d - wd)) <= 1e-9 * scale
    # a direct double loop on a few lags
    for a in sorted({0, min(1, flen - 1), flen // 2, flen - 1}):
        want = sum(int(xi[k]) * int(xi[k - a]) for k in range(a, n))
        assert int(S.exact_corr(yi, xi, flen)[0][a]) == want


def test_exact_corr_asserts_its_precondition():
    big = np.full(48001, 20000, np.int64)
    big[0] = 2 ** 20
    with pytest.raises(AssertionError):
        S.exact_corr(big, big, 4)
    with pytest.raises(AssertionError):
        S.exact_corr(np.ones(4), np.ones(4), 2)                 # floats, not int64


def _ill_conditioned(n):
    """Autocorrelation of a strongly coloured signal: condition number about 1e5 at n = 512."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal(6000)
    for _ in range(3):
        x = np.convolve(x, [1.0, 1.9, 1.0])[:6000]
    xi, _ = S.int16_values(x)
    yi, _ = S.int16_values(np.convolve(x, [0.5, 0.3])[:6000] + 0.05 * np.std(x) * rng.standard_normal(6000))
    return S.exact_corr_f64(yi, xi, n)


@pytest.mark.parametrize("n", [1, 2, 64, 512])
def test_levinson_mp_residual(n):
    r, d = _ill_conditioned(n)
    c = S.levinson_mp(r, d)
    assert len(c) == n
    res = S.residual_mp(r, d, c)
    print("levinson_mp n=%d: relative residual %s, cond %.2e" % (n, mpmath.nstr(res, 3),
                                                                 np.linalg.cond(S.toeplitz(r))))
    assert res < mpmath.mpf("1e-40")
    lu = np.linalg.solve(S.toeplitz(r), d)
    assert np.linalg.norm(S.mp_to_f64(c) - lu) <= 1e-16 * np.linalg.cond(S.toeplitz(r)) * 100 * np.linalg.norm(lu)
    ld = S.mp_to_ld(c)
    assert ld.dtype == np.longdouble and np.array_equal(ld.astype(np.float64), S.mp_to_f64(c))


def test_scaled_residual_is_exact():
    r, d = _ill_conditioned(64)
    c = np.linalg.solve(S.toeplitz(r), d)
    got = S.scaled_residual(r, d, c)
    with mpmath.workdps(60):
        T = mpmath.matrix(S.toeplitz(r).tolist())
        res = T * mpmath.matrix(c.tolist()) - mpmath.matrix(d.tolist())
        top = max(abs(v) for v in res)
        want = top / (mpmath.mpf(float(np.max(np.sum(np.abs(S.toeplitz(r)), axis=1)))) * float(np.max(np.abs(c)))
                      + float(np.max(np.abs(d))))
    assert abs(got - float(want)) <= 1e-12 * float(want)
    assert 0 < got < 1e-15
    assert S.scaled_residual(r, d, np.zeros(64)) == 1.0        # c = 0: ||d|| / ||d||
    lead = S.scaled_residual(r, d, np.linalg.solve(S.toeplitz(r[:10]), d[:10]))      # a leading system
    assert 0 <= lead < 1e-15


def test_project_ld_against_a_direct_sum_and_its_bound():
    rng = np.random.default_rng(8)
    n, flen = 700, 33
    (yi, y32), (xi, x32) = _pair(rng, n)
    c = rng.standard_normal(flen) * np.exp(-np.arange(flen) / 5.0)
    num, den, Bn, Bd = S.project_ld(y32, x32, c)
    with mpmath.workdps(50):
        x = [mpmath.mpf(float(v)) for v in x32]
        y = [mpmath.mpf(float(v)) for v in y32] + [mpmath.mpf(0)] * (flen - 1)
        cm = [mpmath.mpf(float(v)) for v in c]
        s = [mpmath.fsum(cm[a] * x[k - a] for a in range(flen) if 0 <= k - a < n) for k in range(n + flen - 1)]
        wnum = mpmath.fsum(v * v for v in s)
        wden = mpmath.fsum((a - b) ** 2 for a, b in zip(y, s))
        assert abs(mpmath.mpf(float(num)) - wnum) <= 1e-15 * wnum      # float(): long double -> double costs 1e-16
        assert abs(mpmath.mpf(float(den)) - wden) <= 1e-15 * wden
    assert Bn >= float(num) and Bd >= float(den)
    # plain float64 evaluation in another order stays inside the bound, and the bound is not vacuous
    s64 = np.convolve(x32.astype(np.float64), c)
    e64 = np.concatenate([y32.astype(np.float64), np.zeros(flen - 1)])
    for have, want, B in ((np.sum(s64 * s64), num, Bn), (np.sum((e64 - s64) ** 2), den, Bd)):
        tol = S.projection_bound(n, flen, B)
        assert abs(float(np.longdouble(have) - want)) <= tol
        assert tol <= 1e-13 * B
    assert S.project_ld(y32[:0], x32[:0], c)[:2] == (0, 0)
    assert S.gamma(4) == 4 * S.U / (1 - 4 * S.U)


def test_oracle_db_error_on_the_families():
    """|oracle.sdr_db - dB of project_ld at the mpmath solution| over the eight families of test_gpu_sdr at flen =
    512: the oracle's own error, which sets the score tolerance of test_gpu_sdr_stages.py.  Measured 8.6e-13 dB
    (recorded there as ORACLE_VS_MP_DB); four times what is measured here must stay within the tolerance in use."""
    import test_gpu_sdr as T
    import test_gpu_sdr_stages as G
    E, X = T._families()
    worst = 0.0
    for i in range(E.shape[0]):
        r, d = S.exact_corr_f64(S.as_int16_values(E[i]), S.as_int16_values(X[i]), 512)
        num, den, _, _ = S.project_ld(E[i], X[i], S.mp_to_ld(S.levinson_mp(r, d)))
        worst = max(worst, abs(O.sdr_db(E[i], X[i], flen=512) - S.db(num, den)))
    print("max |oracle.sdr_db - mp| over the families = %.3e dB" % worst)
    assert 4.0 * worst <= G.SCORE_TOL_DB
    assert G.SCORE_TOL_DB == max(4 * G.ORACLE_VS_MP_DB, 1e-9)
