"""SDR on the device (csrc/sdr.hip, include/drnmf_sdr.h) on the MI355X: the batched Levinson-Durbin solve against
numpy's dense fp64 solve, and the ragged SDR against oracle.sdr_db per row -- never against the code under test."""
import numpy as np
import pytest
import torch

from oracle import drnmf_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 16000
N3 = 3 * FS


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _toeplitz(r):
    n = r.shape[0]
    return r[np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])]


def _int16_values(x):
    """Scaled to a peak of 20000 and rounded to integers: what a 16-bit file holds, as float32 in [-1, 1)."""
    x = np.round(x / np.max(np.abs(x)) * 20000.0)
    return (x / 32768.0).astype(np.float32)


def _ar(rng, n, poles):
    """White noise through the all-pole filter with the given (conjugate-closed) poles."""
    a = np.real(np.poly(poles))
    x = rng.standard_normal(n + 2000)
    y = np.zeros_like(x)
    for i in range(len(x)):
        acc = x[i]
        for k in range(1, len(a)):
            if i - k >= 0:
                acc -= a[k] * y[i - k]
        y[i] = acc
    return y[2000:]


def _families(seed=11, n=N3):
    """The eight reference families: four AR-coloured, amplitude-modulated 'speech-like' signals (poles 0.97,
    0.9 e^{+-0.3i} and 0.95 e^{+-0.1k i}, k = 1..4), a 440 Hz sine, a period-100 sequence, white noise and a
    400-sample burst in silence; each estimate is the reference through a 40-tap decaying filter plus noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    refs = []
    for k in range(1, 5):
        poles = [0.97, 0.9 * np.exp(0.3j), 0.9 * np.exp(-0.3j), 0.95 * np.exp(0.1j * k), 0.95 * np.exp(-0.1j * k)]
        am = 0.55 + 0.45 * np.sin(2 * np.pi * (2.0 + k) * t / FS + k)
        refs.append(_ar(rng, n, poles) * am)
    refs.append(np.sin(2 * np.pi * 440.0 * t / FS))
    refs.append(np.tile(rng.standard_normal(100), n // 100 + 1)[:n])
    refs.append(rng.standard_normal(n))
    burst = np.zeros(n)
    burst[n // 3:n // 3 + 400] = rng.standard_normal(400)
    refs.append(burst)
    refs = [_int16_values(x) for x in refs]
    ests = []
    for x in refs:
        hfilt = rng.standard_normal(40) * np.exp(-np.arange(40) / 8.0)
        y = np.convolve(x.astype(np.float64), hfilt)[:n]
        y = y + 0.1 * np.sqrt(np.mean(y ** 2)) * rng.standard_normal(n)
        ests.append(_int16_values(y))
    return np.stack(ests), np.stack(refs)


@pytest.mark.parametrize("n", [1, 2, 31, 512, 2048])
def test_toeplitz_solve_well_conditioned(ops, n):
    """r = autocorrelation of white noise (condition number about 2), random d, 7 systems: c within 1e-10
    (relative, max norm) of np.linalg.solve -- fp64 eps times a few thousand operations is below 1e-12."""
    rng = np.random.default_rng(100 + n)
    r = np.empty((7, n))
    for k in range(7):
        x = rng.standard_normal(4 * 2048)
        r[k] = [np.dot(x[a:], x[:len(x) - a]) for a in range(n)]
    d = rng.standard_normal((7, n)) * r[:, :1]
    c, info = ops.toeplitz_solve(_t(r), _t(d))
    c, info = c.cpu().numpy(), info.cpu().numpy()
    assert info.dtype == np.int32 and np.all(info == 0), info
    worst = 0.0
    for k in range(7):
        want = np.linalg.solve(_toeplitz(r[k]), d[k])
        worst = max(worst, float(np.max(np.abs(c[k] - want)) / np.max(np.abs(want))))
    print("toeplitz_solve n=%d: max relative error %.3e" % (n, worst))
    assert worst <= 1e-10, worst
    c1, info1 = ops.toeplitz_solve(_t(r[3]), _t(d[3]))           # 1-D in, 1-D out, same bits as in the batch
    assert c1.shape == (n,) and np.array_equal(c1.cpu().numpy(), c[3]) and int(info1[0]) == 0


def test_toeplitz_solve_flags(ops):
    """info = 1 (c = 0) for r[0] <= 0 or not finite; info = 2 + k with the order-k solution, zero-extended, when
    the prediction error stops being positive at step k (r = 1, 1, 1, ...: rank one, stops at step 1)."""
    n = 6
    r = np.zeros((4, n))
    r[1, 0] = -1.0
    r[2, 0] = np.inf
    r[3] = 1.0
    d = np.ones((4, n))
    c, info = ops.toeplitz_solve(_t(r), _t(d))
    c, info = c.cpu().numpy(), info.cpu().numpy()
    assert info.tolist() == [1, 1, 1, 3]
    assert np.all(c[:3] == 0.0)
    assert c[3].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("flen", [512, 32])
def test_sdr_device_solver_vs_oracle_badly_conditioned(ops, flen):
    """The eight families (condition numbers up to 1.9e9 at flen = 512): solver='device' within 1e-2 dB of
    oracle.sdr_db and of solver='host' per row, info = 0 everywhere."""
    E, X = _families()
    got, coef, en, info = ops.sdr_db(_t(E), _t(X), flen=flen, return_parts=True, solver="device")
    host = ops.sdr_db(_t(E), _t(X), flen=flen).cpu().numpy()
    got, info = got.cpu().numpy(), info.cpu().numpy()
    want = np.array([O.sdr_db(E[i], X[i], flen=flen) for i in range(E.shape[0])])
    print("sdr[flen=%d]: max |device - oracle| = %.3e dB, max |device - host| = %.3e dB, max |host - oracle| "
          "= %.3e dB" % (flen, np.max(np.abs(got - want)), np.max(np.abs(got - host)),
                         np.max(np.abs(host - want))))
    print("   device:", got.tolist())
    print("   oracle:", want.tolist())
    assert np.all(info == 0), info
    assert coef.shape == (8, flen) and en.shape == (8, 2)
    for i in range(E.shape[0]):
        assert abs(float(got[i]) - want[i]) <= 1e-2, (i, float(got[i]), want[i])
        assert abs(float(got[i]) - float(host[i])) <= 1e-2, (i, float(got[i]), float(host[i]))


RAGGED_LENGTHS = [100, 511, 513, 4097, 8192, 8193, 20011, 33333, N3]


def test_sdr_ragged_rows_vs_oracle_and_bitwise(ops):
    """9 rows of 100 samples (shorter than flen) to 3 s, junk behind each row's length: every row within 1e-2 dB
    of the oracle on the row's own samples; coef, energies and dB bitwise equal alone at the row's own width, in
    the batch, and in a batch of another stride and order."""
    E, X = _families(seed=12)
    rng = np.random.default_rng(13)
    E = np.concatenate([E, E[6:7]])
    X = np.concatenate([X, X[6:7]])
    lens = np.array(RAGGED_LENGTHS)
    Ej, Xj = E.copy(), X.copy()
    for i, n in enumerate(lens):                              # junk, not zeros, behind the row
        Ej[i, n:] = rng.standard_normal(N3 - n)
        Xj[i, n:] = 3.0 * rng.standard_normal(N3 - n)
    got = ops.sdr_db(_t(Ej), _t(Xj), return_parts=True, lengths=lens, solver="device")
    db, coef, en, info = (t.cpu().numpy() for t in got)
    assert np.all(info == 0), info
    worst = 0.0
    for i, n in enumerate(lens):
        want = O.sdr_db(E[i, :n], X[i, :n])
        worst = max(worst, abs(float(db[i]) - want))
        print("   row %d len %d: device %.6f oracle %.6f" % (i, n, float(db[i]), want))
    print("sdr ragged: max |device - oracle| = %.3e dB" % worst)
    for i, n in enumerate(lens):
        assert abs(float(db[i]) - O.sdr_db(E[i, :n], X[i, :n])) <= 1e-2, (i, n)
    # alone, at its own width
    for i, n in enumerate(lens):
        a = ops.sdr_db(_t(E[i:i + 1, :n]), _t(X[i:i + 1, :n]), return_parts=True, solver="device")
        a_db, a_coef, a_en, a_info = (t.cpu().numpy() for t in a)
        assert np.array_equal(a_db[0], db[i]) and np.array_equal(a_coef[0], coef[i]), (i, n)
        assert np.array_equal(a_en[0], en[i]) and a_info[0] == 0
    # another stride, another position, other junk; lengths as a device tensor
    order = np.array([4, 8, 0, 6, 2, 7, 1, 3, 5])
    E2 = rng.standard_normal((9, N3 + 777)).astype(np.float32)
    X2 = rng.standard_normal((9, N3 + 777)).astype(np.float32)
    for k, i in enumerate(order):
        E2[k, :lens[i]], X2[k, :lens[i]] = E[i, :lens[i]], X[i, :lens[i]]
    b = ops.sdr_db(_t(E2), _t(X2), return_parts=True, lengths=_t(lens[order]), solver="device")
    b_db, b_coef, b_en, b_info = (t.cpu().numpy() for t in b)
    assert np.array_equal(b_db, db[order]) and np.array_equal(b_coef, coef[order])
    assert np.array_equal(b_en, en[order]) and np.all(b_info == 0)
    # lengths=None is the full stride
    full = ops.sdr_db(_t(E[:3]), _t(X[:3]), solver="device").cpu().numpy()
    same = ops.sdr_db(_t(E[:3]), _t(X[:3]), lengths=[N3] * 3, solver="device").cpu().numpy()
    assert np.array_equal(full, same)
    with pytest.raises(ValueError):
        ops.sdr_db(_t(E[:3]), _t(X[:3]), lengths=[N3 + 1, 5, 5], solver="device")
    with pytest.raises(ValueError):
        ops.sdr_db(_t(E[:3]), _t(X[:3]), lengths=[5, 5], solver="device")


def test_sdr_silent_and_empty_rows(ops):
    """A silent reference with a live estimate, a silent pair, and a row of length 0 (junk behind it): info = 1,
    coefficients 0, and the dB the host solver gives for the same zero-padded pairs (-inf, NaN, NaN).  A live row
    next to them is untouched."""
    rng = np.random.default_rng(21)
    n = 6000
    E = np.zeros((4, n), np.float32)
    X = np.zeros((4, n), np.float32)
    E[0] = 0.1 * rng.standard_normal(n)
    E[2], X[2] = rng.standard_normal(n), rng.standard_normal(n)          # row 2 has length 0: junk
    X[3] = 0.3 * rng.standard_normal(n)
    E[3] = X[3] + 0.05 * rng.standard_normal(n)
    lens = np.array([n, n, 0, n])
    db, coef, en, info = (t.cpu().numpy() for t in
                          ops.sdr_db(_t(E), _t(X), return_parts=True, lengths=lens, solver="device"))
    assert info.tolist() == [1, 1, 1, 0]
    assert np.all(coef[:3] == 0.0) and np.any(coef[3] != 0.0)
    Ez, Xz = E.copy(), X.copy()
    Ez[2], Xz[2] = 0.0, 0.0
    host = ops.sdr_db(_t(Ez), _t(Xz)).cpu().numpy()
    assert np.array_equal(db[:3], host[:3], equal_nan=True), (db, host)
    assert db[0] == -np.inf and np.isnan(db[1]) and np.isnan(db[2])
    assert abs(float(db[3]) - O.sdr_db(E[3], X[3])) <= 1e-2
    assert abs(float(db[3]) - float(host[3])) <= 1e-2


def test_compute_scores_with_the_device_solver(ops):
    """Ragged lengths_est / lengths_ref: column 0 within 1e-2 dB of the default call, columns 1-5 identical to it
    (NaNs included)."""
    E, X = _families(seed=14)
    n_ref = [N3, N3 - 4000, 30000, 20000, N3, 41000, 16000, N3 - 1]
    n_est = [N3 - 300, N3, 30000, 26000, 47000, 40000, 16500, N3]
    S0, labels0 = ops.compute_scores(_t(E), _t(X), FS, lengths_est=n_est, lengths_ref=n_ref)
    S1, labels1 = ops.compute_scores(_t(E), _t(X), FS, lengths_est=n_est, lengths_ref=n_ref, sdr_solver="device")
    assert labels0 == labels1 and S1.shape == (8, 6) and S1.dtype == np.float64
    print("compute_scores: max |SDR device - host| = %.3e dB" % np.max(np.abs(S1[:, 0] - S0[:, 0])))
    assert np.all(np.abs(S1[:, 0] - S0[:, 0]) <= 1e-2), (S1[:, 0], S0[:, 0])
    assert np.array_equal(S1[:, 1:], S0[:, 1:], equal_nan=True)
    assert np.all(np.isfinite(S1[:, :2])) and np.all(np.isnan(S1[:, 2:5]))
    for i in range(8):
        m = min(n_est[i], n_ref[i])
        assert abs(S1[i, 0] - O.sdr_db(E[i, :m], X[i, :m])) <= 1e-2, i


def test_enhance_passes_the_solver_through(ops):
    """model.enhance(..., ref=, sdr_solver='device'): the same waveforms as without the argument, S[:, 0] within
    1e-2 dB, the other columns identical."""
    from drnmf_amd import layers
    F, r, K = 257, 16, 3
    P = O.synth_problem(2, 4, F, r, seed=3)
    N = 2 * r
    params = dict(input_dim=F, hidden_dim=N, output_dim=F, mask_value=-1., maxseq=200, K_layers=K,
                  W=P["W"], alph=N / 4.0, lam1=0.3, params_untied=["log_D", "log_alph"],
                  params_trainable=["log_D", "log_alph"])
    model = layers.build_unfolded_snmf(params, device=DEV)
    rng = np.random.default_rng(4)
    lens = rng.integers(int(0.3 * FS), int(1.5 * FS), size=6)
    noisy = [(rng.standard_normal(n) * 3000 * (1 + 0.5 * np.sin(np.arange(n) / 900.0))).astype(np.int16)
             for n in lens]
    clean = [(0.6 * w + 200 * rng.standard_normal(len(w))).astype(np.int16) for w in noisy]
    out0, S0, labels0 = model.enhance(noisy, N=512, hop=128, batch_size=4, ref=clean, fs=FS)
    out1, S1, labels1 = model.enhance(noisy, N=512, hop=128, batch_size=4, ref=clean, fs=FS, sdr_solver="device")
    assert labels0 == labels1
    for a, b in zip(out0, out1):
        assert np.array_equal(a, b)
    print("enhance: max |SDR device - host| = %.3e dB" % np.max(np.abs(S1[:, 0] - S0[:, 0])))
    assert np.all(np.abs(S1[:, 0] - S0[:, 0]) <= 1e-2), (S1[:, 0], S0[:, 0])
    assert np.array_equal(S1[:, 1:], S0[:, 1:], equal_nan=True)
