"""STOI on the MI355X (csrc/stoi.hip) against the fp64 restatement in stoi_ref.py [STOI-memory], and the
compute_scores row (score_audio.m:177-238)."""
import numpy as np
import pytest
import torch

import stoi_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _batch(fs, seed, lengths):
    """Rows: clean speech-like references; estimates = the reference plus noise at -5, 0, 5, 10 dB and a
    low-passed, delayed copy (cycled over the rows)."""
    rng = np.random.default_rng(seed)
    refs, ests = [], []
    for i, n in enumerate(lengths):
        x = R.speech_like(rng, n, fs).astype(np.float32)
        kind = i % 5
        y = R.lowpass_delay(x, 23) if kind == 4 else R.add_noise(rng, x, (-5, 0, 5, 10)[kind])
        refs.append(x)
        ests.append(y.astype(np.float32))
    width = max(lengths)
    E = np.zeros((len(lengths), width), np.float32)
    X = np.zeros((len(lengths), width), np.float32)
    for i, n in enumerate(lengths):
        E[i, :n], X[i, :n] = ests[i], refs[i]
    return E, X


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("fs", [8000, 10000, 16000])
def test_stoi_matches_the_oracle(ops, fs):
    lengths = [int(fs * s) for s in (2.6, 3.1, 1.9, 2.2, 2.8, 3.4)]
    E, X = _batch(fs, 10 + fs // 1000, lengths)
    got, parts = ops.stoi(_dev(E), _dev(X), fs=fs, lengths=lengths, return_parts=True)
    got = got.cpu().numpy()
    keep = parts["keep"].cpu().numpy()
    env_r, env_e = parts["env_ref"].cpu().numpy(), parts["env_est"].cpu().numpy()
    errs = []
    for i, n in enumerate(lengths):
        want, P = R.stoi(X[i, :n].astype(np.float64), E[i, :n].astype(np.float64), fs, return_parts=True)
        e = P["energies"]
        # no frame near the threshold: the keep decision cannot legitimately differ between fp32 and fp64
        assert np.min(np.abs(e - e.max() + R.DYN_RANGE)) > 1e-3
        nv = len(P["keep"])
        assert np.array_equal(keep[i, :nv], P["keep"]), i
        assert not keep[i, nv:].any()
        nf = P["env_ref"].shape[0]
        assert nf >= 30 and int(parts["n_kept"][i]) == nf + 1
        for g, w in ((env_r[i, :nf], P["env_ref"]), (env_e[i, :nf], P["env_est"])):
            rel = np.abs(g - w) / np.abs(w)
            assert float(rel.max()) <= 1e-4, (i, float(rel.max()))
        errs.append(abs(float(got[i]) - want))
        assert abs(float(got[i]) - want) <= 1e-4, (i, float(got[i]), want)
    print("fs=%d max |STOI - oracle| = %.3e" % (fs, max(errs)))


def test_ragged_rows_equal_rows_scored_alone_and_runs_repeat(ops):
    fs = 16000
    lengths = [int(fs * s) for s in (1.3, 3.7, 0.9, 2.4, 0.01, 3.0, 2.0)]
    E, X = _batch(fs, 5, lengths)
    e, x = _dev(E), _dev(X)
    a = ops.stoi(e, x, fs=fs, lengths=lengths).cpu().numpy()
    b = ops.stoi(e, x, fs=fs, lengths=lengths).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    for i, n in enumerate(lengths):
        alone = ops.stoi(_dev(E[i, :n]), _dev(X[i, :n]), fs=fs).cpu().numpy()
        assert alone.tobytes() == a[i:i + 1].tobytes(), i
    assert np.isnan(a[4])                             # 10 ms: not one frame
    assert np.all(np.isfinite(a[[0, 1, 3, 5, 6]]))


def test_edge_cases_follow_the_oracle(ops):
    fs = 10000
    rng = np.random.default_rng(7)
    x = R.speech_like(rng, fs * 3, fs, gaps=False).astype(np.float32)
    short = x[:128 * 29 + 256].copy()                 # 29 band frames at most
    zero_stretch = x.copy()
    zero_stretch[fs:2 * fs] = 0.0                     # the estimate is silent for a second
    rows = [(x, x), (short, short), (zero_stretch, x), (np.zeros_like(x), x)]
    width = len(x)
    E = np.zeros((len(rows), width), np.float32)
    X = np.zeros((len(rows), width), np.float32)
    lengths = []
    for i, (ee, xx) in enumerate(rows):
        E[i, :len(ee)], X[i, :len(xx)] = ee, xx
        lengths.append(len(xx))
    got = ops.stoi(_dev(E), _dev(X), fs=fs, lengths=lengths).cpu().numpy()
    assert abs(float(got[0]) - 1.0) <= 1e-6
    assert np.isnan(got[1]) and np.isnan(R.stoi(short, short, fs))
    for i in (2, 3):
        want = R.stoi(X[i].astype(np.float64), E[i].astype(np.float64), fs)
        assert abs(float(got[i]) - want) <= 1e-4, (i, float(got[i]), want)
    assert abs(float(got[3]) - 1.0) <= 1e-6           # sum Y^2 = 0 everywhere: Matlab's min gives d = 1
    with pytest.raises(ValueError):
        ops.stoi(_dev(E), _dev(X), fs=44100, lengths=lengths)


def test_compute_scores_row(ops):
    fs = 16000
    rng = np.random.default_rng(9)
    n_ref = [int(fs * s) for s in (2.1, 2.6, 1.8)]
    n_est = [n_ref[0] + 300, n_ref[1] - 500, n_ref[2]]          # longer, shorter, equal
    refs = [R.speech_like(rng, n, fs).astype(np.float32) for n in n_ref]
    ests = []
    for i, n in enumerate(n_est):
        base = np.zeros(n, np.float32)
        m = min(n, n_ref[i])
        base[:m] = refs[i][:m]
        ests.append(R.add_noise(rng, base.astype(np.float64), 5.0 * i).astype(np.float32))
    E = np.zeros((3, max(n_est) + 64), np.float32)
    X = np.zeros((3, max(n_ref) + 16), np.float32)
    for i in range(3):
        E[i, :n_est[i]], X[i, :n_ref[i]] = ests[i], refs[i]
    S, labels = ops.compute_scores(_dev(E), _dev(X), fs, lengths_est=n_est, lengths_ref=n_ref)
    assert labels == ['SDR', 'SNR', 'SegSNR local', 'SegSNR global', 'PESQ', 'STOI']
    assert S.dtype == np.float64 and S.shape == (3, 6)
    assert np.isnan(S[:, 2:5]).all()
    from oracle import drnmf_oracle as O
    for i in range(3):
        m = min(n_est[i], n_ref[i])
        e, x = ests[i][:m].astype(np.float64), refs[i][:m].astype(np.float64)
        snr = 10 * np.log10(np.sum(x ** 2) / np.sum((x - e) ** 2))
        assert abs(S[i, 1] - snr) <= 1e-3, (i, S[i, 1], snr)
        assert abs(S[i, 0] - O.sdr_db(e, x)) <= 1e-2, (i, S[i, 0])
        assert abs(S[i, 5] - R.stoi(x, e, fs)) <= 1e-4, (i, S[i, 5])
