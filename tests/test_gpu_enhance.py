"""The ragged enhancement path on the MI355X (include/drnmf_enhance.h): ops.stft_ragged / istft_ragged /
to_int16_wav_rows against the oracle's stft_mc / reconstruct per row, the reference's own stored vectors, bitwise
batch independence, and model.enhance against the path composed of the per-utterance entry points."""
import math

import numpy as np
import pytest
import torch

from oracle import drnmf_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(512, 128), (1024, 256), (64, 16)]


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _lengths(hop):
    return [1, hop - 1, hop, hop + 1, 3 * hop + 7, 9999, 16001]


def _batch(lens, seed, int16, stride=None):
    """Rows of noise, each valid up to its length and followed by junk the kernels must not read as signal; the
    stride is odd."""
    rng = np.random.default_rng(seed)
    stride = stride or (max(lens) + 1 if max(lens) % 2 == 0 else max(lens) + 2)
    assert stride % 2 == 1
    if int16:
        a = rng.integers(-20000, 20000, size=(len(lens), stride)).astype(np.int16)
    else:
        a = (0.3 * rng.standard_normal((len(lens), stride))).astype(np.float32)
    return a


def _as_float(row):
    return O.wav_int16_to_float(row) if row.dtype == np.int16 else row


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("int16", [True, False], ids=["int16", "float32"])
@pytest.mark.parametrize("N,hop", SIZES)
def test_stft_ragged_matches_stft_mc_per_row(ops, N, hop, int16):
    lens = _lengths(hop)
    pcm = _batch(lens, N + int16, int16)
    idx = [5, 0, 6, 3, 2]                                     # shuffled, part of the batch
    T = max(O.stft_frames(lens[i], N, hop) for i in idx) + 5
    x, re, im, nf = ops.stft_ragged(_t(pcm), lens, sig_index=idx, T=T, N=N, hop=hop, mask_value=-1.0)
    x, re, im = x.cpu().numpy(), re.cpu().numpy(), im.cpu().numpy()
    assert x.shape == (len(idx), T, N // 2 + 1)
    w = O.sqrt_hann(N)
    for k, i in enumerate(idx):
        assert nf[k] == O.stft_frames(lens[i], N, hop)
        S = O.stft_mc(_as_float(pcm[i, :lens[i]]), N, hop, w)
        scale = np.max(np.abs(S))
        n = int(nf[k])
        assert np.max(np.abs(re[k, :n].T - S.real)) <= 2e-5 * scale
        assert np.max(np.abs(im[k, :n].T - S.imag)) <= 2e-5 * scale
        mag = np.sqrt(re[k, :n].astype(np.float64) ** 2 + im[k, :n].astype(np.float64) ** 2)
        assert np.max(np.abs(x[k, :n] - mag)) <= 2e-5 * scale
        assert np.all(x[k, n:] == np.float32(-1.0))
    # another padding value, the default gather list and T
    x2, _, _, nf2 = ops.stft_ragged(_t(pcm), lens, N=N, hop=hop, mask_value=-7.5)
    assert x2.shape[:2] == (len(lens), max(nf2))
    x2 = x2.cpu().numpy()
    for i in range(len(lens)):
        assert np.all(x2[i, int(nf2[i]):] == np.float32(-7.5))
        assert np.all(x2[i, :int(nf2[i])] >= 0)


@pytest.mark.parametrize("crop", [False, True], ids=["full", "crop"])
@pytest.mark.parametrize("N,hop", SIZES)
def test_istft_ragged_matches_reconstruct_per_row(ops, N, hop, crop):
    lens = _lengths(hop)
    pcm = _batch(lens, 3 * N + 1, False)
    idx = [6, 1, 4, 0, 5, 2]
    rng = np.random.default_rng(N)
    x, re, im, nf = ops.stft_ragged(_t(pcm), lens, sig_index=idx, N=N, hop=hop)
    T, F = x.shape[1], N // 2 + 1
    mask = rng.random((len(idx), T, F)).astype(np.float32)
    width = 16001 + 2 * hop + 3
    out = torch.full((len(lens), width), 7.0, dtype=torch.float32, device=DEV)
    y = ops.istft_ragged(re, im, _t(mask), lens, N, hop, sig_index=idx, out=out, crop=crop).cpu().numpy()
    w = O.sqrt_hann(N)
    n_out = ops.ragged_out_lengths(lens, N, hop, crop)
    for k, i in enumerate(idx):
        S = O.stft_mc(pcm[i, :lens[i]], N, hop, w)
        ref = O.reconstruct(S.real, S.imag, mask[k, :int(nf[k])].T.astype(np.float64), hop, w,
                            lens[i] if crop else None)
        assert ref.shape[0] == n_out[i] == (lens[i] if crop else -(-lens[i] // hop) * hop)
        assert np.max(np.abs(y[i, :n_out[i]] - ref)) <= 1e-4 * np.max(np.abs(ref))
        assert np.all(y[i, n_out[i]:] == 0.0)
    assert np.all(y[3] == 7.0)                                # a row the gather list does not name is untouched
    # the allocating form
    y2 = ops.istft_ragged(re, im, _t(mask), lens, N, hop, sig_index=idx, crop=crop)
    assert y2.shape == (len(lens), max(n_out))
    for i in idx:
        assert torch.equal(y2[i, :n_out[i]].cpu(), torch.from_numpy(y[i, :n_out[i]]))


@pytest.mark.parametrize("N", [512, 1024, 64])
def test_unmasked_round_trip(ops, N):
    hop = N // 4
    lens = _lengths(hop)
    pcm = _batch(lens, N + 11, False)
    _, re, im, _ = ops.stft_ragged(_t(pcm), lens, N=N, hop=hop)
    y = ops.istft_ragged(re, im, None, lens, N, hop, crop=True).cpu().numpy()
    for i, n in enumerate(lens):
        err = np.max(np.abs(y[i, :n] - pcm[i, :n])) / np.max(np.abs(pcm[i, :n]))
        assert err <= 1e-4, (i, err)


@pytest.mark.parametrize("int16", [True, False], ids=["int16", "float32"])
@pytest.mark.parametrize("N,hop", SIZES)
def test_a_row_is_bitwise_independent_of_its_batch(ops, N, hop, int16):
    lens = _lengths(hop)
    pcm = _batch(lens, 17 + N, int16)
    rng = np.random.default_rng(1)
    F = N // 2 + 1
    nfs = [O.stft_frames(n, N, hop) for n in lens]
    masks = [rng.random((nf, F)).astype(np.float32) for nf in nfs]

    def run(rows, T, order):
        """Signals `rows` as a batch of their own (other strides, positions and T); returns per signal
        (x, re, im, y, q)."""
        sub = np.zeros((len(rows), max(lens[i] for i in rows) + 3), pcm.dtype)
        sl = [lens[i] for i in rows]
        for r, i in enumerate(rows):
            sub[r, :lens[i]] = pcm[i, :lens[i]]
        x, re, im, nf = ops.stft_ragged(_t(sub), sl, sig_index=order, T=T, N=N, hop=hop)
        m = np.zeros(tuple(x.shape), np.float32)
        for k, r in enumerate(order):
            m[k, :nf[k]] = masks[rows[r]]
        y = ops.istft_ragged(re, im, _t(m), sl, N, hop, sig_index=order)
        n_out = ops.ragged_out_lengths(sl, N, hop)
        q = ops.to_int16_wav_rows(y * 3.0, n_out)
        res = {}
        for k, r in enumerate(order):
            n = int(nf[k])
            res[rows[r]] = tuple(a.cpu().numpy() for a in (x[k, :n], re[k, :n], im[k, :n], y[r, :n_out[r]],
                                                           q[r, :n_out[r]]))
        return res

    full = run(list(range(len(lens))), max(nfs), list(range(len(lens))))
    other = run([6, 2, 4, 1, 5], max(nfs) + 37, [3, 0, 4, 2, 1])
    for i in range(len(lens)):
        alone = run([i], nfs[i], [0])[i]
        for name, a, b in zip("x re im y q".split(), full[i], alone):
            assert a.tobytes() == b.tobytes(), (i, name)
        if i in other:
            for name, a, b in zip("x re im y q".split(), full[i], other[i]):
                assert a.tobytes() == b.tobytes(), (i, name)


def test_int16_rows_equal_the_per_file_conversion(ops):
    rng = np.random.default_rng(9)
    lens = [1, 127, 4000, 16001, 9999]
    y = (0.2 * rng.standard_normal((len(lens), 16003))).astype(np.float32)
    y[1] *= 9.0                                               # loud rows: peak > 1
    y[3] *= 30.0
    y[2, 3999] = 1.0                                          # a peak of exactly 1 is not divided
    y[0, 5] = 50.0                                            # behind row 0's length: not part of its peak
    yd = _t(y)
    q = ops.to_int16_wav_rows(yd, lens)
    assert q.dtype == torch.int16 and tuple(q.shape) == y.shape
    for k, n in enumerate(lens):
        want = ops.to_int16_wav(yd[k, :n].contiguous())
        assert torch.equal(q[k, :n], want), k
        assert int(q[k, n:].abs().max()) == 0
    peaks = [np.max(np.abs(y[k, :n])) for k, n in enumerate(lens)]
    assert peaks[1] > 1 and peaks[3] > 1 and peaks[4] < 1 and peaks[0] < 1
    assert int(q[3].abs().max()) == 32767


def test_ragged_inverse_matches_reference_golden(ops, golden):
    """The reference's own vectors (util.istft_mc(flag_noDiv=1) executed as written, tests/golden) as a one-row
    batch, at the tolerance of test_reconstruction_kernels_match_reference_golden."""
    g = golden
    re, im = _t(g["istft_S_re"].T[None].astype(np.float32)), _t(g["istft_S_im"].T[None].astype(np.float32))
    hop = int(g["istft_hop"])
    nf, F = re.shape[1], re.shape[2]
    N = 2 * (F - 1)
    full = g["istft_mc_x"][0]
    # a length whose frame count is the stored spectrogram's and whose output is the stored signal's
    n = full.shape[0]
    assert O.stft_frames(n, N, hop) == nf and ops.ragged_out_lengths([n], N, hop)[0] == n
    y = ops.istft_ragged(re, im, None, [n], N, hop).cpu().numpy()[0]
    assert np.max(np.abs(y[:n] - full)) <= 1e-4 * np.max(np.abs(full))
    want = g["istft_mc_x_nsampl100"][0]
    mask = _t(g["istft_mask"].T[None].astype(np.float32))
    ym = ops.istft_ragged(re, im, mask, [n], N, hop).cpu().numpy()[0]
    assert np.max(np.abs(ym[:100] - want)) <= 1e-4 * np.max(np.abs(want))


def test_ops_reject_bad_arguments(ops):
    pcm = _t(np.zeros((3, 1001), np.int16))
    with pytest.raises(ValueError):
        ops.stft_ragged(pcm, [10, 0, 5])                      # a length of 0
    with pytest.raises(ValueError):
        ops.stft_ragged(pcm, [10, 1002, 5])
    with pytest.raises(ValueError):
        ops.stft_ragged(pcm, [10, 20])
    with pytest.raises(ValueError):
        ops.stft_ragged(pcm, [10, 20, 30], sig_index=[0, 3])
    with pytest.raises(ValueError):
        ops.stft_ragged(pcm, [10, 20, 1000], T=3)
    with pytest.raises(ValueError):
        ops.stft_ragged(pcm.double(), [10, 20, 30])
    with pytest.raises(ValueError):
        ops.stft_ragged(pcm.cpu(), [10, 20, 30])
    x, re, im, _ = ops.stft_ragged(pcm, torch.tensor([10, 20, 30]), N=64, hop=16)
    with pytest.raises(ValueError):
        ops.istft_ragged(re, im[:, :, :5], None, [10, 20, 30], 64, 16)
    with pytest.raises(ValueError):
        ops.istft_ragged(re, im, x[:2], [10, 20, 30], 64, 16)
    with pytest.raises(ValueError):
        ops.istft_ragged(re, im, None, [10, 20, 30], 64, 16, sig_index=[0, 1])
    with pytest.raises(ValueError):
        ops.to_int16_wav_rows(torch.zeros((3, 50), device=DEV), [10, 0, 5])
    with pytest.raises(ValueError):
        ops.to_int16_wav_rows(torch.zeros((3, 50), device=DEV), [10, 51, 5])


# ---- model.enhance -------------------------------------------------------------------------------------------
N_E, HOP_E, F_E = 512, 128, 257


def _utterances(seed=4):
    rng = np.random.default_rng(seed)
    lens = rng.integers(int(0.3 * 16000), int(1.5 * 16000), size=12)
    noisy = [(rng.standard_normal(n) * 3000 * (1 + 0.5 * np.sin(np.arange(n) / 900.0))).astype(np.int16)
             for n in lens]
    clean = [(0.6 * w + 200 * rng.standard_normal(len(w))).astype(np.int16) for w in noisy]
    return noisy, clean


def _snmf_model():
    from drnmf_amd import layers
    r, K = 16, 3
    P = O.synth_problem(2, 4, F_E, r, seed=3)
    N = 2 * r
    params = dict(input_dim=F_E, hidden_dim=N, output_dim=F_E, mask_value=-1., maxseq=200, K_layers=K,
                  W=P["W"], alph=N / 4.0, lam1=0.3, params_untied=["log_D", "log_alph"],
                  params_trainable=["log_D", "log_alph"])
    return layers.build_unfolded_snmf(params, device=DEV)


def _lstm_model():
    from drnmf_amd import layers
    torch.manual_seed(0)
    np.random.seed(0)
    return layers.build_lstm(dict(mask_value=-1., maxseq=200, input_dim=F_E, output_dim=F_E, K_layers=2,
                                  hidden_dim=48), device=DEV)


def _composed(ops, model, noisy, batch_size):
    """The enhancement loop out of the per-utterance entry points: ops.stft each, -1 padding on the host,
    model.predict, then ops.istft_masked and ops.to_int16_wav each."""
    specs, mags = [], []
    for w in noisy:
        re, im, mag = ops.stft(_t(w), N=N_E, hop=HOP_E, want_mag=True)
        specs.append((re, im))
        mags.append(mag[0].cpu().numpy())
    nfs = [m.shape[0] for m in mags]
    x = np.full((len(noisy), max(nfs), F_E), -1.0, np.float32)
    for i, m in enumerate(mags):
        x[i, :nfs[i]] = m
    masks = model.predict(x, batch_size=batch_size)
    ys, qs = [], []
    for i, w in enumerate(noisy):
        n_out = -(-len(w) // HOP_E) * HOP_E
        m = _t(masks[i:i + 1, :nfs[i]])
        y = ops.istft_masked(specs[i][0], specs[i][1], m, n_out, N_E, HOP_E)
        ys.append(y[0].cpu().numpy())
        qs.append(ops.to_int16_wav(y[0]).cpu().numpy())
    return ys, qs, [masks[i, :nfs[i]] for i in range(len(noisy))]


def _rel(a, b):
    return max(float(np.max(np.abs(x - y))) / float(np.max(np.abs(y))) for x, y in zip(a, b))


@pytest.mark.parametrize("family", ["snmf", "lstm"])
def test_enhance_equals_the_composed_path(ops, family):
    """model.enhance (12 utterances of 0.3 - 1.5 s, batch_size=5: three slabs of different T) against the path
    composed of the existing per-utterance entry points.

    The two differ by the model's batch-shape dependence (the GEMMs tile a slab by its row count), which is
    measured here first: d = the largest relative-to-peak difference between two composed runs that differ only
    in predict's batch_size (12 against 1).  The assertion is enhance within bound = max(4 d, 1e-4) of the
    batch_size=12 run (never tighter than the inverse transform's own 1e-4), int16 within 1 + ceil(32767 bound),
    masks within bound.  Measured on the MI355X (fp32 matrix mode): d = 1.8e-7 (snmf) and
    3.3e-8 (lstm), so bound = 1e-4 and the int16 tolerance is 5; enhance itself lands 1.8e-7 / 1.9e-7 from the
    composed run."""
    model = _snmf_model() if family == "snmf" else _lstm_model()
    noisy, clean = _utterances()
    y12, q12, m12 = _composed(ops, model, noisy, 12)
    y1, _, m1 = _composed(ops, model, noisy, 1)
    d = _rel(y1, y12)
    bound = max(4.0 * d, 1e-4)
    d_mask = max(float(np.max(np.abs(a - b))) for a, b in zip(m1, m12))
    yf, masks = model.enhance(noisy, N=N_E, hop=HOP_E, batch_size=5, dtype='float32', return_masks=True)
    e_y, e_m = _rel(yf, y12), max(float(np.max(np.abs(a - b))) for a, b in zip(masks, m12))
    print("enhance[%s]: batch-shape dependence d = %.3e (masks %.3e), bound = %.3e; enhance vs composed = %.3e "
          "(masks %.3e)" % (family, d, d_mask, bound, e_y, e_m))
    assert len(yf) == 12
    for i, w in enumerate(noisy):
        assert yf[i].dtype == np.float32 and yf[i].shape == (-(-len(w) // HOP_E) * HOP_E,)
        assert masks[i].shape == m12[i].shape
    assert e_y <= bound, (e_y, bound)
    assert e_m <= bound, (e_m, bound)
    q = model.enhance(noisy, N=N_E, hop=HOP_E, batch_size=5)
    tol = 1 + int(math.ceil(32767 * bound))
    for i in range(12):
        assert q[i].dtype == np.int16 and q[i].shape == q12[i].shape
        assert int(np.max(np.abs(q[i].astype(int) - q12[i].astype(int)))) <= tol
    # cropped to the utterance, and from a padded 2-D array with lengths=
    lens = [len(w) for w in noisy]
    packed = np.zeros((12, max(lens)), np.int16)
    for i, w in enumerate(noisy):
        packed[i, :lens[i]] = w
    qc = model.enhance(packed, N=N_E, hop=HOP_E, batch_size=5, crop=True, lengths=lens)
    qd = model.enhance(_t(packed), N=N_E, hop=HOP_E, batch_size=12, crop=True, lengths=lens)
    for i in range(12):
        assert qc[i].shape == (lens[i],)
        assert int(np.max(np.abs(qc[i].astype(int) - qd[i].astype(int)))) <= tol
    # the score rows
    out, S, labels = model.enhance(noisy, N=N_E, hop=HOP_E, batch_size=5, ref=clean, fs=16000)
    for a, b in zip(out, q):
        assert np.array_equal(a, b)
    n_out = [len(a) for a in out]
    est = np.zeros((12, max(n_out)), np.float32)
    ref = np.zeros((12, max(lens)), np.float32)
    for i in range(12):
        est[i, :n_out[i]] = out[i].astype(np.float32) / np.float32(32768.0)
        ref[i, :lens[i]] = clean[i].astype(np.float32) / np.float32(32768.0)
    S2, labels2 = ops.compute_scores(_t(est), _t(ref), 16000, n_out, lens)
    assert labels == labels2 == ops.SCORE_LABELS
    assert S.shape == (12, 6) and np.array_equal(S, S2, equal_nan=True)
    assert np.all(np.isnan(S[:, 2:5])) and np.all(np.isfinite(S[:, :2]))


def test_enhance_rejects_what_it_cannot_do(ops):
    model = _snmf_model()
    noisy, _ = _utterances()
    with pytest.raises(ValueError):
        model.enhance(noisy[:2], N=1024, hop=256)             # 513 bins for a 257-bin model
    model.cell.stateful = True
    try:
        with pytest.raises(NotImplementedError):
            model.enhance(noisy[:2], N=N_E, hop=HOP_E)
    finally:
        model.cell.stateful = False
    with pytest.raises(NotImplementedError):
        model_l = _lstm_model()
        model_l._stateful = lambda: True
        model_l.enhance(noisy[:2], N=N_E, hop=HOP_E)
