"""STOI (csrc/stoi.hip) at the shapes its kernels branch on: more rows than one lengths-upload launch holds, rows
long enough for several frames per thread in the silence scan, and every resampling ratio stoi_rate accepts beyond
8 and 16 kHz.  Everything is compared with stoi_ref.stoi per row at the tolerances of test_gpu_stoi.py; the inputs
are built here once, and a CPU test checks on the oracle alone that they satisfy the comparison's preconditions."""
import functools

import numpy as np
import pytest

import stoi_ref as R

gpu = pytest.mark.gpu

RATES = [6250, 12000, 20000, 24000, 32000, 48000]
LONG_ROWS = [(16000, 12.0), (8000, 12.0), (10000, 30.0)]      # frames per thread in the silence scan: 4, 4, 10
N_ROWS = 230                                                   # > ST_LEN_CHUNK = 224
MANY_FS = 16000
MANY_SECONDS = (2.0, 2.3, 1.7, 2.6, 1.9, 2.15)


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rows(fs, seed, seconds):
    """[(est, ref)] float32: speech-like references; estimates = the reference plus noise at -5, 0, 5, 10 dB or a
    low-passed, delayed copy (cycled over the rows), as test_gpu_stoi._batch."""
    rng = np.random.default_rng(seed)
    rows = []
    for i, s in enumerate(seconds):
        x = R.speech_like(rng, int(round(fs * s)), fs).astype(np.float32)
        kind = i % 5
        y = R.lowpass_delay(x, 23) if kind == 4 else R.add_noise(rng, x, (-5, 0, 5, 10)[kind])
        rows.append((y.astype(np.float32), x))
    return rows


@functools.lru_cache(maxsize=None)
def _inputs():
    """name -> (fs, [(est, ref)]): exactly the rows the GPU tests score."""
    out = {"many": (MANY_FS, _rows(MANY_FS, 31, MANY_SECONDS))}
    for fs, sec in LONG_ROWS:
        out["long%d" % fs] = (fs, _rows(fs, 40 + fs // 1000, (sec, 2.0)))
    for fs in RATES:
        out["rate%d" % fs] = (fs, _rows(fs, 60 + fs // 1000, (2.4, 3.1, 1.8)))
    return out


@functools.lru_cache(maxsize=None)
def _oracle(name):
    fs, rows = _inputs()[name]
    return [R.stoi(x.astype(np.float64), y.astype(np.float64), fs, return_parts=True) for y, x in rows]


def _many_order():
    """230 row indices into the six distinct pairs, shuffled; pair 5 sits only at indices >= 224."""
    rng = np.random.default_rng(2)
    head = rng.permutation(np.arange(224) % 5)
    tail = np.array([5, 2, 5, 0, 5, 4])
    order = np.concatenate([head, tail])
    assert order.shape[0] == N_ROWS and np.all(order[:224] != 5) and set(order.tolist()) == set(range(6))
    return order


@pytest.mark.parametrize("name", ["many"] + ["long%d" % fs for fs, _ in LONG_ROWS] + ["rate%d" % fs for fs in RATES])
def test_inputs_meet_the_preconditions_on_the_oracle(name):
    """CPU only: for every row the GPU tests score, no silence-detector frame lies within 1e-3 dB of the threshold
    (so the keep decision cannot legitimately differ between precisions) and there are at least 30 band frames."""
    for i, (want, P) in enumerate(_oracle(name)):
        e = P["energies"]
        margin = float(np.min(np.abs(e - e.max() + R.DYN_RANGE)))
        assert margin > 1e-3, (name, i, margin)
        assert P["env_ref"].shape[0] >= 30 and np.isfinite(want), (name, i)


def test_long_rows_need_several_frames_per_thread():
    """CPU only: the long rows have the frame counts the silence scan branches on (ceil(nv / 256) = 4, 4, 10)."""
    for (fs, sec), per in zip(LONG_ROWS, (4, 4, 10)):
        nv = len(_oracle("long%d" % fs)[0][1]["keep"])
        assert -(-nv // 256) == per, (fs, nv)


@pytest.mark.parametrize("fs", [8000, 16000] + RATES)
def test_oracle_resampler_against_upfirdn(fs):
    """CPU only: stoi_ref.resample is Matlab's resample(x, 10000, fs) -- upfirdn with stoi_ref.resample_filter's
    taps, the filter delayed so that its centre falls on an output sample, and the delay trimmed -- to 1e-12."""
    from scipy.signal import upfirdn
    rng = np.random.default_rng(fs)
    for n in (1, 37, 1000, 4001):
        x = rng.standard_normal(n)
        h, p, q, half = R.resample_filter(fs)
        nz = int(q - half % q)                                    # Matlab: floor(q - mod(Lhalf, q))
        delay = (half + nz) // q
        ny = -(-n * p // q)
        need = (delay + ny) * q - ((n - 1) * p + len(h) + nz) + q
        hh = np.concatenate([np.zeros(nz), h, np.zeros(max(need, 0))])
        want = upfirdn(hh, x, p, q)[delay:delay + ny]
        got = R.resample(x, fs)
        assert got.shape == want.shape == (ny,)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (fs, n)


def _compare(ops, name, fs, rows, oracle, row_of=None):
    """Score the batch; compare EVERY row with the oracle of its pair (keep mask, n_kept, envelopes, score) at the
    tolerances of test_gpu_stoi.test_stoi_matches_the_oracle.  Returns the device scores and parts (numpy)."""
    row_of = list(range(len(rows))) if row_of is None else list(row_of)
    lengths = [len(rows[k][1]) for k in row_of]
    width = max(lengths)
    E = np.zeros((len(row_of), width), np.float32)
    X = np.zeros((len(row_of), width), np.float32)
    for i, k in enumerate(row_of):
        E[i, :lengths[i]], X[i, :lengths[i]] = rows[k]
    got, parts = ops.stoi(_dev(E), _dev(X), fs=fs, lengths=lengths, return_parts=True)
    got = got.cpu().numpy()
    keep = parts["keep"].cpu().numpy()
    env_r, env_e = parts["env_ref"].cpu().numpy(), parts["env_est"].cpu().numpy()
    n_kept = parts["n_kept"].cpu().numpy()
    worst = 0.0
    for i, k in enumerate(row_of):
        want, P = oracle[k]
        e = P["energies"]
        assert np.min(np.abs(e - e.max() + R.DYN_RANGE)) > 1e-3
        nv = len(P["keep"])
        assert np.array_equal(keep[i, :nv], P["keep"]), (name, i)
        assert not keep[i, nv:].any()
        nf = P["env_ref"].shape[0]
        assert nf >= 30 and int(n_kept[i]) == nf + 1, (name, i, nf, int(n_kept[i]))
        for g, w in ((env_r[i, :nf], P["env_ref"]), (env_e[i, :nf], P["env_est"])):
            rel = np.abs(g - w) / np.abs(w)
            assert float(rel.max()) <= 1e-4, (name, i, float(rel.max()))
        worst = max(worst, abs(float(got[i]) - want))
        assert abs(float(got[i]) - want) <= 1e-4, (name, i, float(got[i]), want)
    print("%s fs=%d: %d rows, max |STOI - oracle| = %.3e" % (name, fs, len(row_of), worst))
    return got, keep, env_r, env_e, n_kept


@gpu
def test_more_rows_than_one_lengths_upload(ops):
    """230 rows (ST_LEN_CHUNK = 224, so the second upload launch runs) built from six distinct pairs in a shuffled
    order, one of them only at indices >= 224: every row against the oracle of its pair, and copies of a pair
    bitwise equal to one another and to the pair scored alone."""
    fs, rows = _inputs()["many"]
    order = _many_order()
    got, keep, env_r, env_e, n_kept = _compare(ops, "many", fs, rows, _oracle("many"), row_of=order)
    for k in range(6):
        y, x = rows[k]
        alone, parts = ops.stoi(_dev(y), _dev(x), fs=fs, return_parts=True)
        alone = alone.cpu().numpy()
        a_keep = parts["keep"].cpu().numpy()[0]
        a_env = parts["env_ref"].cpu().numpy()[0], parts["env_est"].cpu().numpy()[0]
        nf = int(parts["n_kept"][0]) - 1
        where = np.flatnonzero(order == k)
        assert where.size >= 3
        for i in where:
            assert got[i:i + 1].tobytes() == alone.tobytes(), (k, i)
            assert int(n_kept[i]) == nf + 1 and np.array_equal(keep[i, :a_keep.shape[0]], a_keep), (k, i)
            assert env_r[i, :nf].tobytes() == a_env[0][:nf].tobytes(), (k, i)
            assert env_e[i, :nf].tobytes() == a_env[1][:nf].tobytes(), (k, i)


@gpu
@pytest.mark.parametrize("fs,seconds", LONG_ROWS)
def test_long_rows(ops, fs, seconds):
    """12 s at 16 and 8 kHz, 30 s at 10 kHz (4, 4 and 10 frames per thread in the silence scan), each in one batch
    with a 2 s row: keep mask, n_kept, envelopes and score of both rows."""
    name = "long%d" % fs
    _compare(ops, name, fs, _inputs()[name][1], _oracle(name))


@gpu
@pytest.mark.parametrize("fs", RATES)
def test_other_rates(ops, fs):
    """6250 Hz (up-sampling, p/q = 8/5) and 12, 20, 24, 32, 48 kHz (q up to 24): three rows each."""
    name = "rate%d" % fs
    _compare(ops, name, fs, _inputs()[name][1], _oracle(name))


@gpu
@pytest.mark.parametrize("fs", [22050, 11025])
def test_unsupported_rates_raise(ops, fs):
    y, x = _inputs()["rate12000"][1][0]
    with pytest.raises(ValueError):
        ops.stoi(_dev(y), _dev(x), fs=fs)
