"""ESTOI on the MI355X (drnmf_stoi_ext, estoi_segment_kernel in csrc/stoi.hip) against the fp64 restatement in
estoi_ref.py [ESTOI-memory], the kernel alone against the same arithmetic on its own inputs, and the extended
compute_scores row."""
import numpy as np
import pytest
import torch

import estoi_ref as ER
import stoi_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _bits(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("fs", [10000, 16000])
def test_estoi_matches_the_oracle_and_the_kernel_its_own_inputs(ops, fs):
    """Six rows of 1.9 to 3.4 s.  |ESTOI - reference| <= 1e-4 (STOI's bound: the device's envelopes are held to
    1e-4 relative, and perturbing the fp64 envelopes by that much moved ESTOI by at most 1.6e-5 on these rows).
    The new kernel alone: every d_m within 1e-9 of estoi_from_env on the float32 envelopes the device itself
    produced (fp64 on both sides, only the order of a few hundred additions differs), and estoi_out the fp64 mean
    of the downloaded d_ext within 1e-6 (one float32 rounding of a value of at most 1)."""
    lengths, E, X, want = ER.oracle_batch(fs)
    got, parts = ops.estoi(_dev(E), _dev(X), fs, lengths=lengths, return_parts=True)
    assert got.dtype == torch.float32 and got.shape == (6,)
    got = got.cpu().numpy()
    keep = parts["keep"].cpu().numpy()
    env_r, env_e = parts["env_ref"].cpu().numpy(), parts["env_est"].cpu().numpy()
    d_ext = parts["d_ext"].cpu().numpy()
    V = ops.stoi_vad_frames(max(lengths), fs)
    assert d_ext.dtype == np.float64 and d_ext.shape == (6, V - 30)
    err, err_d, err_m = [], [], []
    for i, (val, P) in enumerate(want):
        e = P["energies"]
        # no frame near the threshold: the keep decision cannot legitimately differ between fp32 and fp64
        assert np.min(np.abs(e - e.max() + R.DYN_RANGE)) > 1e-3
        nv = len(P["keep"])
        assert np.array_equal(keep[i, :nv], P["keep"]), i
        nf = P["env_ref"].shape[0]
        assert nf >= 30 and int(parts["n_kept"][i]) == nf + 1
        err.append(abs(float(got[i]) - val))
        again = ER.segment_scores(env_r[i, :nf], env_e[i, :nf])
        assert again.shape == (nf - 29,)
        err_d.append(float(np.max(np.abs(d_ext[i, :nf - 29] - again))))
        err_m.append(abs(float(got[i]) - float(d_ext[i, :nf - 29].mean())))
    print("fs=%d max |ESTOI - oracle| = %.3e, max |d_m - recomputed| = %.3e, max |ESTOI - mean d_ext| = %.3e" %
          (fs, max(err), max(err_d), max(err_m)))
    assert max(err) <= 1e-4, err
    assert max(err_d) <= 1e-9, err_d
    assert max(err_m) <= 1e-6, err_m


def _edge_rows(fs=10000):
    """speech_like(gaps=False) cut to 128 k + 256 samples: k - 1 band frames when every frame is kept."""
    rng = np.random.default_rng(21)
    x = R.speech_like(rng, fs * 3, fs, gaps=False).astype(np.float32)
    y = R.add_noise(rng, x, 5.0).astype(np.float32)
    rows = {}
    for nf in (29, 30, 33, 34):
        n = 128 * (nf + 1) + 256
        rows[nf] = (y[:n].copy(), x[:n].copy())
    return rows, (y, x)


def test_segment_count_edges(ops):
    """nf = 29: no segment, NaN.  30: one live wave.  33: four segments fill the first workgroup.  34: a second
    workgroup with one live wave."""
    fs = 10000
    rows, _ = _edge_rows(fs)
    for nf, (y, x) in rows.items():
        want, P = ER.estoi(x.astype(np.float64), y.astype(np.float64), fs, return_parts=True)
        assert P["env_ref"].shape[0] == nf and P["keep"].all()
        got, parts = ops.estoi(_dev(y), _dev(x), fs, return_parts=True)
        got = float(got.cpu().numpy()[0])
        assert int(parts["n_kept"][0]) == nf + 1
        if nf < 30:
            assert np.isnan(got) and np.isnan(want)
            continue
        assert abs(got - want) <= 1e-4, (nf, got, want)
        d = parts["d_ext"].cpu().numpy()[0]
        assert d.shape == (nf - 29,)
        again = ER.segment_scores(parts["env_ref"].cpu().numpy()[0, :nf], parts["env_est"].cpu().numpy()[0, :nf])
        assert float(np.max(np.abs(d - again))) <= 1e-9, nf


def test_ragged_rows_equal_rows_scored_alone_and_runs_repeat(ops):
    fs = 10000
    rows, (y3, x3) = _edge_rows(fs)
    short = 100                                                   # 10 ms: not one frame
    pairs = [rows[29], rows[30], rows[33], rows[34], (y3[:short], x3[:short]), (y3, x3)]
    lengths = [len(x) for _, x in pairs]
    E = np.zeros((len(pairs), max(lengths)), np.float32)
    X = np.zeros_like(E)
    for i, (y, x) in enumerate(pairs):
        E[i, :len(y)], X[i, :len(x)] = y, x
    e, x = _dev(E), _dev(X)
    a = ops.estoi(e, x, fs, lengths=lengths)
    b = ops.estoi(e, x, fs, lengths=lengths)
    assert _bits(a) == _bits(b)
    a = a.cpu().numpy()
    for i, n in enumerate(lengths):
        alone = ops.estoi(_dev(E[i, :n]), _dev(X[i, :n]), fs).cpu().numpy()
        assert alone.tobytes() == a[i:i + 1].tobytes(), i
    assert np.isnan(a[0]) and np.isnan(a[4])
    assert np.all(np.isfinite(a[[1, 2, 3, 5]]))


def test_edge_semantics_follow_the_oracle(ops):
    """x against x: 1.  An estimate silent for one second: NaN beside a finite STOI from the same call.  An all-zero
    estimate: NaN (STOI: 1, Matlab's min).  The reference gives NaN in the same cases."""
    fs = 10000
    rng = np.random.default_rng(7)
    x = R.speech_like(rng, fs * 3, fs, gaps=False).astype(np.float32)
    zero_stretch = x.copy()
    zero_stretch[fs:2 * fs] = 0.0
    E = np.stack([x, zero_stretch, np.zeros_like(x)])
    X = np.stack([x, x, x])
    s, es = ops.stoi_ext(_dev(E), _dev(X), fs)
    s, es = s.cpu().numpy(), es.cpu().numpy()
    want = [ER.estoi(X[i].astype(np.float64), E[i].astype(np.float64), fs, return_parts=True) for i in range(3)]
    assert abs(float(es[0]) - 1.0) <= 1e-6 and abs(want[0][0] - 1.0) <= 1e-12
    assert np.isnan(es[1]) and np.isnan(want[1][0])
    assert np.isfinite(s[1]) and abs(float(s[1]) - want[1][1]["stoi"]) <= 1e-4
    assert np.isnan(es[2]) and np.isnan(want[2][0])
    assert abs(float(s[2]) - 1.0) <= 1e-6
    with pytest.raises(ValueError):
        ops.estoi(_dev(E), _dev(X), 44100)


def test_one_call_gives_both_scores(ops):
    fs = 16000
    lengths, E, X, _ = ER.oracle_batch(fs)
    e, x = _dev(E), _dev(X)
    s, es = ops.stoi_ext(e, x, fs, lengths=lengths)
    assert _bits(s) == _bits(ops.stoi(e, x, fs=fs, lengths=lengths))
    assert _bits(es) == _bits(ops.estoi(e, x, fs, lengths=lengths))
    assert _bits(es) == _bits(ops.stoi(e, x, fs=fs, lengths=lengths, extended=True))
    only_s, none = ops.stoi_ext(e, x, fs, lengths=lengths, want_estoi=False)
    assert none is None and _bits(only_s) == _bits(s)
    assert float((s - es).abs().min()) > 1e-3                    # two numbers, not one twice
    with pytest.raises(ValueError):
        ops.stoi_ext(e, x, fs, lengths=lengths, want_stoi=False, want_estoi=False)


def _score_inputs(fs=16000):
    rng = np.random.default_rng(9)
    n_ref = [int(fs * s) for s in (2.1, 2.6, 1.8)]
    n_est = [n_ref[0] + 300, n_ref[1] - 500, n_ref[2]]          # longer, shorter, equal
    E = np.zeros((3, max(n_est) + 64), np.float32)
    X = np.zeros((3, max(n_ref) + 16), np.float32)
    for i in range(3):
        x = R.speech_like(rng, n_ref[i], fs).astype(np.float32)
        base = np.zeros(n_est[i], np.float32)
        m = min(n_est[i], n_ref[i])
        base[:m] = x[:m]
        E[i, :n_est[i]] = R.add_noise(rng, base.astype(np.float64), 5.0 * i).astype(np.float32)
        X[i, :n_ref[i]] = x
    return E, X, n_est, n_ref


@pytest.mark.parametrize("solver", ["host", "device"])
def test_extended_compute_scores_row(ops, solver):
    fs = 16000
    E, X, n_est, n_ref = _score_inputs(fs)
    S6, labels6 = ops.compute_scores(_dev(E), _dev(X), fs, lengths_est=n_est, lengths_ref=n_ref, sdr_solver=solver)
    S, labels = ops.compute_scores(_dev(E), _dev(X), fs, lengths_est=n_est, lengths_ref=n_ref, sdr_solver=solver,
                                   extended=True)
    assert labels6 == ops.SCORE_LABELS and S6.shape == (3, 6)
    assert labels == ops.SCORE_LABELS + ['ESTOI'] and labels[-1] == 'ESTOI'
    assert S.dtype == np.float64 and S.shape == (3, 7)
    assert np.array_equal(S[:, :6], S6, equal_nan=True)
    assert S[:, :6].tobytes() == S6.tobytes()                    # NaNs included: the same bits
    m = [min(a, b) for a, b in zip(n_est, n_ref)]
    w = max(m)
    Et, Xt = np.zeros((3, w), np.float32), np.zeros((3, w), np.float32)
    for i in range(3):
        Et[i, :m[i]], Xt[i, :m[i]] = E[i, :m[i]], X[i, :m[i]]
    direct = ops.estoi(_dev(Et), _dev(Xt), fs, lengths=m).cpu().numpy()
    assert np.array_equal(S[:, 6], direct.astype(np.float64))
    for i in range(3):
        want = ER.estoi(Xt[i, :m[i]].astype(np.float64), Et[i, :m[i]].astype(np.float64), fs)
        assert abs(S[i, 6] - want) <= 1e-4, (i, S[i, 6], want)


def test_enhance_returns_the_extended_row(ops):
    from drnmf_amd import layers
    torch.manual_seed(0)
    np.random.seed(0)
    model = layers.build_lstm(dict(mask_value=-1., maxseq=200, input_dim=257, output_dim=257, K_layers=2,
                                   hidden_dim=48), device="cuda:0")
    rng = np.random.default_rng(4)
    lens = [int(1.0 * 16000), int(1.4 * 16000), int(1.2 * 16000)]
    clean = [(R.speech_like(rng, n, 16000) * 32767).astype(np.int16) for n in lens]
    noisy = [(c + 1500 * rng.standard_normal(len(c))).astype(np.int16) for c in clean]
    out6, S6, labels6 = model.enhance(noisy, batch_size=2, ref=clean, fs=16000)
    out, S, labels = model.enhance(noisy, batch_size=2, ref=clean, fs=16000, extended_scores=True)
    assert labels6 == ops.SCORE_LABELS and labels == ops.SCORE_LABELS + ['ESTOI']
    assert S6.shape == (3, 6) and S.shape == (3, 7)
    for a, b in zip(out, out6):
        assert np.array_equal(a, b)
    n_out = [len(a) for a in out]
    est = np.zeros((3, max(n_out)), np.float32)
    ref = np.zeros((3, max(lens)), np.float32)
    for i in range(3):
        est[i, :n_out[i]] = out[i].astype(np.float32) / np.float32(32768.0)
        ref[i, :lens[i]] = clean[i].astype(np.float32) / np.float32(32768.0)
    S2, labels2 = ops.compute_scores(_dev(est), _dev(ref), 16000, n_out, lens, extended=True)
    assert labels2 == labels and np.array_equal(S, S2, equal_nan=True)
    assert np.array_equal(S[:, :6], S6, equal_nan=True)
    assert np.all(np.isfinite(S[:, 6]))
