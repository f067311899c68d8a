"""The STOI criterion on the MI355X (include/drnmf_stoi_loss.h): ops.stoi_loss against ops.stoi (the loss, bit for
bit) and against the fp64 restatement of tests/stoi_loss_ref.py (the gradient), its independence of the batch, and
the models' loss='stoi' on top of it.  Every test prints what it measured before it asserts."""
import functools

import numpy as np
import pytest
import torch

import lstm_ref as LR
import stoi_ref as SR
import stoi_loss_ref as R
from oracle import drnmf_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS_LIST = [10000, 16000, 8000]
# The gradient's bound per fs: 8 x the worst max-norm relative error measured on the MI355X against the fp64
# restatement (9.6e-8, 1.9e-7, 1.3e-7), rounded up to a power of ten; it may not exceed 1e-4.
G_TOL = {10000: 1e-6, 16000: 1e-5, 8000: 1e-5}


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)     # (a copy: the shared references are read-only)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _batch(fs):
    """Every row of the issue's table at fs (and, at 16 kHz, the silent stretch and the all-zero estimate) as one
    ragged batch: (lens, est, ref, [(loss, counted, g) of the fp64 restatement per row]), computed once."""
    pairs = [R.pair(*c) for c in R.CASES if c[2] == fs]
    if fs == 16000:
        pairs.append(R.stretch_pair())
        pairs.append((pairs[0][0], np.zeros_like(pairs[0][1])))
    lens = [len(x) for x, _ in pairs]
    width = max(lens) + 5
    est, ref = np.zeros((len(lens), width), np.float32), np.zeros((len(lens), width), np.float32)
    for i, (x, y) in enumerate(pairs):
        ref[i, :lens[i]], est[i, :lens[i]] = x, y
        est[i, lens[i]:] = 1e30                                      # junk behind the length must not be read
    refs = [R.stoi_loss(x, y, fs) for x, y in pairs]
    for a in (est, ref):
        a.setflags(write=False)
    return lens, est, ref, refs


@pytest.mark.parametrize("fs", FS_LIST)
def test_stoi_loss_matches_stoi_and_the_fp64_gradient(ops, fs):
    lens, est, ref, refs = _batch(fs)
    n = len(lens)
    ed, rd = _t(est), _t(ref)
    loss, counted, g, sums = ops.stoi_loss(ed, rd, lens, fs=fs)
    score = ops.stoi(ed, rd, fs=fs, lengths=lens)
    assert loss.shape == (n,) and counted.shape == (n,) and g.shape == est.shape and sums.shape == (2,)
    assert all(t.dtype == torch.float32 for t in (loss, counted, g, sums))
    lo, co, gn, sm = _np(loss), _np(counted), _np(g), _np(sums)
    tot, cnt, worst = 0.0, 0, 0.0
    for i, m in enumerate(lens):
        rl, rc, rg = refs[i]
        assert co[i] == float(rc), (i, co[i], rc)
        assert np.all(gn[i, m:] == 0.0), (i, "zeros behind the length")
        if not rc:
            assert lo[i] == 0.0 and np.all(gn[i] == 0.0) and not np.isfinite(float(score[i])), i
            print("stoi_loss fs=%d n=%d: not counted" % (fs, m))
            continue
        assert torch.equal(loss[i], -score[i]), (i, float(loss[i]), float(score[i]))
        tot, cnt = tot + rl, cnt + 1
        err = R.rel_err(gn[i, :m], rg)
        print("stoi_loss fs=%d n=%d: loss %.7f (fp64 %.7f), g off by %.3e of max|ref| = %.3e" %
              (fs, m, lo[i], rl, err, np.max(np.abs(rg))))
        assert abs(lo[i] - rl) <= 1e-6 * abs(rl), (i, lo[i], rl)
        assert np.all(np.isfinite(gn[i]))
        worst = max(worst, err)
    print("stoi_loss fs=%d: worst gradient error %.3e (bound %.0e)" % (fs, worst, G_TOL[fs]))
    assert G_TOL[fs] <= 1e-4
    assert worst <= G_TOL[fs], worst
    assert sm[1] == cnt and cnt >= 1
    assert abs(sm[0] - tot) <= 1e-6 * abs(tot)


@pytest.mark.parametrize("fs", FS_LIST)
def test_a_row_alone_and_a_second_run_give_the_batch_bits(ops, fs):
    lens, est, ref, _ = _batch(fs)
    ed, rd = _t(est), _t(ref)
    loss, counted, g, sums = ops.stoi_loss(ed, rd, lens, fs=fs)
    again = ops.stoi_loss(ed, rd, lens, fs=fs)
    for a, b in zip((loss, counted, g, sums), again):
        assert torch.equal(a, b)
    for k, m in enumerate(lens):
        l1, c1, g1, s1 = ops.stoi_loss(_t(est[k:k + 1, :m]), _t(ref[k:k + 1, :m]), [m], fs=fs)
        assert torch.equal(l1[0], loss[k]) and torch.equal(c1[0], counted[k]), k
        assert torch.equal(g1[0], g[k, :m]), (k, float((g1[0] - g[k, :m]).abs().max()))
        assert float(s1[1]) == float(counted[k]) and float(s1[0]) == float(loss[k])
    # nothing counted: sums = {0, 0}
    k = [i for i, m in enumerate(lens) if float(counted[i]) == 0.0]
    if k:
        s0 = ops.stoi_loss(_t(est[k]), _t(ref[k]), [lens[i] for i in k], fs=fs)[3]
        assert _np(s0).tolist() == [0.0, 0.0]


def test_ops_refuse_bad_arguments(ops):
    z = torch.zeros((2, 5000), device=DEV)
    with pytest.raises(ValueError, match="not supported"):
        ops.stoi_loss(z, z, [5000, 4000], fs=44100)
    with pytest.raises(ValueError, match="lengths"):
        ops.stoi_loss(z, z, [5000, 5001])
    with pytest.raises(ValueError, match="lengths"):
        ops.stoi_loss(z, z, [5000])
    with pytest.raises(ValueError, match="stoi_loss: g"):
        ops.stoi_loss(z, z, [5000, 4000], out=(None, None, torch.zeros((2, 4999), device=DEV), None))


# ---- the models' loss='stoi' ------------------------------------------------------------------------------------------
FS = 16000
WAV_LENS = [9000, 7800, 8400, 6600]
WN, WHOP, WF = 64, 16, 33
FAMILIES = ["snmf", "lstm"]


def _build(family, W, seed=0, lr=1e-3, compile_=True):
    """The tiny models of tests/test_gpu_wave_loss.py: the unfolded cell (r = 8, K = 2) or the LSTM (H = 13, K = 2)."""
    from drnmf_amd import layers
    if family == "snmf":
        np.random.seed(seed)
        m = layers.build_unfolded_snmf(dict(input_dim=WF, hidden_dim=8, output_dim=WF, mask_value=-1., maxseq=100,
                                            K_layers=2, W=W, alph=2.0, lam1=0.3,
                                            params_untied=["log_D", "log_alph"],
                                            params_trainable=["log_D", "log_alph"]))
        rng = np.random.default_rng(seed)
        m.set_weights([a + (0.05 * rng.standard_normal(a.shape)).astype(np.float32)
                       if (a.ndim == 2 and a.shape[0] != a.shape[1]) or a.ndim == 1 else a for a in m.get_weights()])
    else:
        m = layers.build_lstm(dict(mask_value=-1.0, maxseq=8, input_dim=WF, output_dim=WF, K_layers=2, hidden_dim=13,
                                   recurrent_activation="sigmoid"), device=torch.device(DEV))
        m.set_weights(LR.random_weights(np.random.default_rng(seed), WF, 13, 2))
    return m.compile(lr=lr) if compile_ else m


@functools.lru_cache(maxsize=None)
def _wav_set():
    """Four speech-like recordings at 16 kHz and their noisy copies (5 dB); the last one has a stretch 60 dB down,
    whose frames the silence detector drops: fewer than 30 band frames are left and the row is never counted."""
    rng = np.random.default_rng(21)
    clean = [SR.speech_like(rng, n, FS, gaps=False) for n in WAV_LENS]
    clean[3][2000:4000] *= 1e-3
    noisy = [SR.add_noise(rng, c, 5.0).astype(np.float32) for c in clean]
    clean = [c.astype(np.float32) for c in clean]
    for a in noisy + clean:
        a.setflags(write=False)
    return noisy, clean, O.synth_problem(2, 100, WF, 4, seed=3, density=0.2)["W"]


def _by_hand(ops, noisy):
    lens = [v.shape[0] for v in noisy]
    pcm = np.zeros((len(lens), max(lens)), np.float32)
    for i, v in enumerate(noisy):
        pcm[i, :lens[i]] = v
    x, re, im, _ = ops.stft_ragged(_t(pcm), lens, N=WN, hop=WHOP, mask_value=-1.0)
    return lens, x, re, im


@pytest.mark.parametrize("family", FAMILIES)
def test_model_gradients_are_those_of_the_hand_written_chain(ops, family):
    noisy, clean, W = _wav_set()
    a, b = _build(family, W), _build(family, W)
    bank = a._wave_bank(list(noisy), list(clean), WN, WHOP, None, "test")
    x, cot_fn = a._wave_batch(bank, np.arange(len(noisy)), WN, WHOP, "stoi", FS)
    flat = a.loss_and_grads_cot(x, cot_fn).clone()

    lens, xh, re, im = _by_hand(ops, noisy)
    assert torch.equal(xh, x)
    ref = torch.zeros((len(lens), max(lens)), device=DEV)
    for i, c in enumerate(clean):
        ref[i, :lens[i]] = _t(c)
    nout = ops.ragged_out_lengths(lens, WN, WHOP, True)
    seen = {}

    def hand(mask):
        y = ops.istft_ragged(re, im, mask, lens, WN, WHOP, crop=True)
        loss, counted, g, sums = ops.stoi_loss(y, ref, nout, fs=FS)
        seen["loss"], seen["counted"] = loss, counted
        return sums, ops.istft_ragged_vjp(g, re, im, lens, WN, WHOP, crop=True)
    step = b._reduce_and_step

    def spy(buf):
        seen["flat"] = buf.clone()
        return step(buf)
    b._reduce_and_step = spy
    got = float(b.train_on_batch_custom(x, hand))
    f = _np(flat)
    print("%s: loss sum %.6f over %g recordings, per row %s, counted %s" %
          (family, f[-4], f[-3], _np(seen["loss"]).tolist(), _np(seen["counted"]).tolist()))
    assert _np(seen["counted"]).tolist() == [1.0, 1.0, 1.0, 0.0]
    assert f[-3] == 3.0 == f[-2] and f[-1] == 0.0 and np.all(np.isfinite(f)) and np.any(f[:-4] != 0.0)
    assert torch.equal(seen["flat"], flat)
    assert abs(got - f[-4] / 3.0) <= 1e-6 * abs(got)


@pytest.mark.parametrize("family", FAMILIES)
def test_test_on_wavs_is_minus_the_mean_stoi_of_the_counted_reconstructions(ops, family):
    noisy, clean, W = _wav_set()
    m = _build(family, W)
    lens, x, re, im = _by_hand(ops, noisy)
    y = ops.istft_ragged(re, im, m.forward(x), lens, WN, WHOP, crop=True)
    ref = torch.zeros_like(y)
    for i, c in enumerate(clean):
        ref[i, :lens[i]] = _t(c)
    s = _np(ops.stoi(y, ref, fs=FS, lengths=lens))
    assert np.isfinite(s).tolist() == [True, True, True, False]
    want = -float(np.mean(s[:3]))
    for bs in (4, 3):
        got = m.test_on_wavs(list(noisy), list(clean), loss="stoi", N=WN, hop=WHOP, batch_size=bs, fs=FS)
        print("%s: test_on_wavs %.7f, minus the mean STOI %.7f (batch_size %d)" % (family, got, want, bs))
        assert abs(got - want) <= 1e-5 * abs(want), (got, want)


@pytest.mark.parametrize("family", FAMILIES)
def test_twenty_steps_on_stoi_lower_it(ops, family):
    """Only that the gradient points the right way (values in DESIGN.md section 6j); no quality is claimed."""
    noisy, clean, W = _wav_set()
    m = _build(family, W, lr=1e-3)
    before = m.test_on_wavs(list(noisy), list(clean), loss="stoi", N=WN, hop=WHOP, fs=FS)
    for _ in range(20):
        last = m.train_on_wavs(list(noisy), list(clean), loss="stoi", N=WN, hop=WHOP, fs=FS)
    after = m.test_on_wavs(list(noisy), list(clean), loss="stoi", N=WN, hop=WHOP, fs=FS)
    print("%s: -STOI %.5f before, %.5f after 20 full-batch steps at lr 1e-3 (last step's loss %.5f)" %
          (family, before, after, float(last)))
    assert after < before


def test_models_refuse_as_for_si_sdr(ops):
    from drnmf_amd import layers
    noisy, clean, W = _wav_set()
    noisy, clean = list(noisy), list(clean)
    kw = dict(loss="stoi", N=WN, hop=WHOP, fs=FS)
    m = _build("snmf", W, compile_=False)
    for call in (m.train_on_wavs, m.fit_waveform):
        with pytest.raises(ValueError, match="compile"):
            call(noisy, clean, **kw)
    m.compile()
    with pytest.raises(ValueError, match="loss must be"):
        m.train_on_wavs(noisy, clean, loss="estoi", N=WN, hop=WHOP)
    with pytest.raises(ValueError, match="not supported"):
        m.train_on_wavs(noisy, clean, loss="stoi", N=WN, hop=WHOP, fs=44100)
    lstm = layers.build_lstm(dict(mask_value=-1.0, maxseq=8, input_dim=WF, output_dim=WF, K_layers=1, hidden_dim=13,
                                  stateful=True), device=torch.device(DEV))
    lstm.compile()
    for call in (lstm.train_on_wavs, lstm.test_on_wavs, lstm.fit_waveform):
        with pytest.raises(NotImplementedError, match="stateful"):
            call(noisy, clean, **kw)
    h16 = layers.build_lstm(dict(mask_value=-1.0, maxseq=8, input_dim=WF, output_dim=WF, K_layers=1, hidden_dim=32,
                                 operand_dtype="float16"), device=torch.device(DEV))
    with pytest.raises(NotImplementedError):
        h16.compile()
    with pytest.raises(ValueError, match="compile"):
        h16.train_on_wavs(noisy, clean, **kw)
    snmf = layers.build_snmf(dict(r=4, sparsity=0.1, cf='ed', max_iter=2, conv_eps=0., random_seed=1),
                             np.ones((WF, 8), np.float32), device=DEV)
    for call in (snmf.train_on_wavs, snmf.test_on_wavs, snmf.fit_waveform):
        with pytest.raises(NotImplementedError, match="SparseNMFModel"):
            call(noisy, clean, **kw)
