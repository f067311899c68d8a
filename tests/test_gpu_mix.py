"""The device-side mixer on the MI355X (include/drnmf_mix.h): ops.mix_forward against the fp64 reference of
tests/mix_ref.py at block edges, wraps and both sample types, its degenerate rows, the bitwise independence of a
signal from its batch, ops.MixBank against wavs_to_tensors / wavs_to_frames on the downloaded mixtures, and
fit_mixtures / from_mixtures against fit / from_wavs on the same draws.

Bounds (reasoned from the formats, checked on the host against the reference rounded to float32 before any GPU
run): g is an fp64 value rounded once to float32 (2^-24 = 6e-8 relative; 2e-7 allowed); a sample is one fused
multiply-add of float32 values with that g, so it is within 2^-24 (the gain) + 2^-24 (the result's rounding) of
|s| + |g seg|, 2^-22 allowed; the realised SNR of the float32 mixtures within 1e-3 dB of the request."""
import numpy as np
import pytest
import torch

import mix_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPEECH_LENS = [1, 2, 7, 4095, 4096, 4097, 10000]
NOISE_LENS = [1, 3, 7, 4096, 5000, 50000]
SCALES = [1e-3, 0.1, 0.5]


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _signal(rng, n, scale, int16):
    v = scale * rng.standard_normal(n)
    if not int16:
        return v.astype(np.float32)
    v = np.clip(np.round(v * 32768.0), -32768, 32767).astype(np.int16)
    v[v == 0] = 1                                   # no all-zero signal or segment by accident
    return v


def _pack(rows, stride, fill):
    """[n][stride] with `fill` behind every row's length: values the kernels must never use."""
    out = np.full((len(rows), stride), fill, dtype=rows[0].dtype)
    for i, v in enumerate(rows):
        out[i, :len(v)] = v
    return out


_batches = {}


def _batch(n_sig, s_int16, n_int16, stride_s):
    """n_sig signals over the six noise recordings: lengths, scales, offsets (0, L - 1, the middle, a negative one
    and one >= L) and noise indices cycle at different periods, SNRs are uniform in [-10, 20] dB.  Built once per
    key with its fp64 reference and never modified."""
    key = (n_sig, s_int16, n_int16, stride_s)
    if key not in _batches:
        rng = np.random.default_rng(1000 * n_sig + 10 * s_int16 + n_int16)
        noise = [_signal(rng, L, SCALES[(j + 1) % 3], n_int16) for j, L in enumerate(NOISE_LENS)]
        lens = [SPEECH_LENS[(i + (6 if n_sig == 1 else 0)) % 7] for i in range(n_sig)]
        speech = [_signal(rng, n, SCALES[i % 3], s_int16) for i, n in enumerate(lens)]
        idx = np.array([(5 * i + i // 6) % 6 for i in range(n_sig)], dtype=np.int32)
        L = np.array(NOISE_LENS, dtype=np.int64)[idx]
        k = np.arange(n_sig) // 2 % 5
        off = np.select([k == 0, k == 1, k == 2, k == 3], [0 * L, L - 1, L // 2, -3 - L], 2 * L + 5).astype(np.int64)
        snr = rng.uniform(-10.0, 20.0, size=n_sig).astype(np.float32)
        ref = [R.mix_one(speech[i], noise[idx[i]], off[i], snr[i]) for i in range(n_sig)]
        assert stride_s >= max(lens)
        _batches[key] = dict(speech=speech, noise=noise, lens=np.array(lens, dtype=np.int64), idx=idx, off=off, snr=snr,
                             ref=ref, stride_s=stride_s)
    return _batches[key]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(ops, b, speech_energy="given", noise_stride=None, **kw):
    """mix_forward on a batch; the rows are padded with a large value behind their lengths."""
    sp = _pack(b["speech"], b["stride_s"], 30000 if b["speech"][0].dtype == np.int16 else 1e30)
    nz = _pack(b["noise"], noise_stride or max(len(v) for v in b["noise"]),
               30000 if b["noise"][0].dtype == np.int16 else 1e30)
    sp_d, ls_d = _dev(sp), _dev(b["lens"])
    es = ops.mix_energy(sp_d, ls_d) if speech_energy == "given" else None
    noisy, gain = ops.mix_forward(sp_d, ls_d, _dev(nz), _dev(np.array([len(v) for v in b["noise"]], dtype=np.int64)),
                                  _dev(b["idx"]), _dev(b["off"]), _dev(b["snr"]), speech_energy=es, return_gain=True,
                                  **kw)
    return noisy.cpu().numpy(), gain.cpu().numpy(), (None if es is None else es.cpu().numpy())


def _check_against_reference(b, noisy, gain, energy):
    worst = dict(g=0.0, sample=0.0, snr=0.0)
    for i, (g_ref, ref, seg) in enumerate(b["ref"]):
        n = int(b["lens"][i])
        s = R.as_float(b["speech"][i])
        assert g_ref > 0 and np.isfinite(gain[i])
        eg = abs(float(gain[i]) - g_ref) / g_ref
        bound = 2.0 ** -22 * (np.abs(s) + np.abs(g_ref * seg))
        err = np.abs(noisy[i, :n].astype(np.float64) - ref)
        es = float(np.max(err / np.maximum(bound, 1e-300)))
        d = abs(R.realised_snr_db(s, noisy[i, :n].astype(np.float64)) - float(b["snr"][i]))
        worst = dict(g=max(worst["g"], eg), sample=max(worst["sample"], es), snr=max(worst["snr"], d))
        assert eg <= 2e-7, (i, eg)
        assert np.all(err <= bound), (i, es)
        assert d <= 1e-3, (i, d)
        assert not noisy[i, n:].any(), i                                   # exactly 0 behind the length
        if energy is not None:
            assert abs(energy[i] - np.sum(s * s)) <= 1e-13 * np.sum(s * s), i
    print("worst: gain %.3g relative, sample %.3g of its bound, realised SNR %.3g dB off" %
          (worst["g"], worst["sample"], worst["snr"]))


@pytest.mark.parametrize("n_sig,stride_s", [(1, 10001), (5, 4100), (70, 10001), (70, 10000)])
@pytest.mark.parametrize("n_int16", [True, False], ids=["noise-int16", "noise-float32"])
@pytest.mark.parametrize("s_int16", [True, False], ids=["speech-int16", "speech-float32"])
def test_mixtures_match_the_fp64_reference(ops, s_int16, n_int16, n_sig, stride_s):
    b = _batch(n_sig, s_int16, n_int16, stride_s)
    if n_sig == 70:
        assert len(set(b["lens"].tolist())) == 7 and len(set(b["idx"].tolist())) == 6      # repeated noise indices
        assert len(set(zip(b["idx"].tolist(), (np.arange(70) // 2 % 5).tolist()))) >= 25  # offsets x recordings
    noisy, gain, energy = _run(ops, b)
    assert noisy.shape == (n_sig, stride_s) and noisy.dtype == np.float32 and np.isfinite(noisy).all()
    _check_against_reference(b, noisy, gain, energy)


def test_degenerate_rows_are_the_speech_itself(ops):
    rng = np.random.default_rng(3)
    for s_int16 in (True, False):
        n = 5000
        sp = [_signal(rng, n, 0.1, s_int16) for _ in range(9)]
        sp[0] = np.zeros(n, sp[0].dtype)                                   # all-zero speech
        noise = [_signal(rng, 6000, 0.1, False), np.zeros(300, np.float32), _signal(rng, 50, 0.1, False)]
        noise[0][1000:1000 + n] = 0.0                                      # an all-zero segment from offset 1000
        len_n = np.array([6000, 300, 0], dtype=np.int64)                   # the third recording has length 0
        idx = np.array([0, 0, 1, 2, -1, 3, 0, 0, 0], dtype=np.int32)
        off = np.array([7, 1000, 11, 0, 0, 0, 5, 5, 5], dtype=np.int64)
        snr = np.array([3, 3, 3, 3, 3, 3, np.nan, np.inf, -np.inf], dtype=np.float32)
        sp_d, ls_d = _dev(_pack(sp, n + 3, 0)), _dev(np.full(9, n, dtype=np.int64))
        noisy, gain = ops.mix_forward(sp_d, ls_d, _dev(_pack(noise, 6000, 1e30)), _dev(len_n), _dev(idx), _dev(off),
                                      _dev(snr), return_gain=True)
        noisy, gain = noisy.cpu().numpy(), gain.cpu().numpy()
        assert np.array_equal(gain, np.zeros(9, np.float32)), gain
        assert np.isfinite(noisy).all() and not noisy[:, n:].any()
        want = np.stack([R.as_float(v).astype(np.float32) for v in sp])
        assert np.array_equal(noisy[:, :n].view(np.uint32), want.view(np.uint32))
        # and the rows are live: the same speech at a finite SNR over the non-zero part is mixed
        live = ops.mix_forward(sp_d, ls_d, _dev(_pack(noise, 6000, 1e30)), _dev(len_n), _dev(np.zeros(9, np.int32)),
                               _dev(np.full(9, 7, dtype=np.int64)), _dev(np.full(9, 3, dtype=np.float32)),
                               return_gain=True)[1].cpu().numpy()
        assert live[0] == 0 and (live[1:] > 0).all()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n_int16", [True, False], ids=["noise-int16", "noise-float32"])
@pytest.mark.parametrize("s_int16", [True, False], ids=["speech-int16", "speech-float32"])
def test_a_signal_does_not_depend_on_its_batch(ops, s_int16, n_int16):
    b = _batch(70, s_int16, n_int16, 10001)
    noisy, gain, energy = _run(ops, b)
    # a second call, and the speech energy computed inside the call
    again = _run(ops, b)
    inside = _run(ops, b, speech_energy=None)
    for other in (again, inside):
        assert np.array_equal(_bits(other[0]), _bits(noisy)) and np.array_equal(_bits(other[1]), _bits(gain))
    assert np.array_equal(again[2], energy)
    # a larger stride on both sides (aligned rows where they were not)
    wide = _run(ops, dict(b, stride_s=10004), noise_stride=50003)
    assert np.array_equal(_bits(wide[0][:, :10001]), _bits(noisy)) and np.array_equal(_bits(wide[1]), _bits(gain))
    assert not wide[0][:, 10001:].any() and np.array_equal(wide[2], energy)
    # alone, at another position, and with its recording at another index of a larger noise bank
    for i in (0, 3, 12, 32, 69):                      # 1, 4095, 4097, 4096 and 10000 samples
        one = dict(b, speech=[b["speech"][i]], lens=b["lens"][i:i + 1], idx=b["idx"][i:i + 1], off=b["off"][i:i + 1],
                   snr=b["snr"][i:i + 1], stride_s=len(b["speech"][i]))
        n = len(b["speech"][i])
        got = _run(ops, one)
        assert np.array_equal(_bits(got[0][0]), _bits(noisy[i, :n])) and _bits(got[1])[0] == _bits(gain)[i], i
        assert got[2][0] == energy[i]
    perm = np.roll(np.arange(70), 17)
    bank = [b["noise"][5]] + b["noise"] + [b["noise"][0][:1]]
    moved = dict(b, speech=[b["speech"][p] for p in perm], lens=b["lens"][perm], idx=(b["idx"][perm] + 1).astype(np.int32),
                 off=b["off"][perm], snr=b["snr"][perm], noise=bank)
    got = _run(ops, moved)
    assert np.array_equal(_bits(got[0]), _bits(noisy[perm])) and np.array_equal(_bits(got[1]), _bits(gain[perm]))


def test_more_than_65535_signals(ops):
    """The launches are cut into slices of 65 535 rows: 70 000 short signals, seven distinct ones repeated, give
    the bits of the first seven everywhere, and those are the reference's."""
    rng = np.random.default_rng(8)
    n_sig, period, stride = 70000, 7, 9
    speech = [_signal(rng, n, 0.1, False) for n in (9, 1, 5, 8, 2, 7, 3)]
    noise = [_signal(rng, 4, 0.1, True), _signal(rng, 11, 0.5, True)]
    idx, off = np.arange(period, dtype=np.int32) % 2, np.array([0, 3, -2, 10, 5, 1, 40], dtype=np.int64)
    snr = rng.uniform(-10.0, 20.0, size=period).astype(np.float32)
    reps = n_sig // period
    tile = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))
    lens = np.array([len(v) for v in speech], dtype=np.int64)
    noisy, gain = ops.mix_forward(_dev(tile(_pack(speech, stride, 1e30))), _dev(tile(lens)), _dev(_pack(noise, 11, 30000)),
                                  _dev(np.array([4, 11], dtype=np.int64)), _dev(tile(idx)), _dev(tile(off)),
                                  _dev(tile(snr)), return_gain=True)
    noisy, gain = noisy.cpu().numpy(), gain.cpu().numpy()
    assert np.array_equal(_bits(noisy), _bits(tile(noisy[:period]))) and np.array_equal(_bits(gain), _bits(tile(gain[:period])))
    b = dict(ref=[R.mix_one(speech[i], noise[idx[i]], off[i], snr[i]) for i in range(period)], lens=lens, speech=speech,
             snr=snr)
    _check_against_reference(b, noisy[:period], gain[:period], None)


# ---- the bank ----------------------------------------------------------------------------------------------
def _recordings(seed, n_clean=6, int16=True):
    rng = np.random.default_rng(seed)
    lens = rng.integers(300, 1500, size=n_clean)
    lens[0], lens[1] = 1499, 37                                             # an odd stride; shorter than one window
    clean = [_signal(rng, int(n), 0.1, int16) for n in lens]
    noise = [_signal(rng, int(n), 0.05, not int16) for n in (2000, 333, 5)]
    return clean, noise


@pytest.fixture(scope="module")
def bank(ops):
    clean, noise = _recordings(21)
    return ops.MixBank(clean, noise, device=DEV)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32),
                                                                                       b.view(torch.int32))


def test_bank_mixes_what_the_reference_mixes(ops, bank):
    clean, noise = _recordings(21)
    draw = bank.draw(snr_db=(-10.0, 20.0), seed=5, epoch=1)
    wavs = bank.wavs(draw)
    clean32 = bank.clean_wavs()
    for i, v in enumerate(wavs):
        assert v.dtype == np.float32 and np.array_equal(clean32[i], R.as_float(clean[i]).astype(np.float32))
        g, ref, seg = R.mix_one(clean[i], noise[draw[0][i]], draw[1][i], draw[2][i])
        assert np.all(np.abs(v - ref) <= 2.0 ** -22 * (np.abs(R.as_float(clean[i])) + np.abs(g * seg))), i
    noisy, lens = bank.mix(draw)
    assert noisy.data_ptr() == bank.mix(bank.draw(seed=6))[0].data_ptr() and lens.tolist() == [len(v) for v in clean]
    for bad in ((draw[0], draw[1]), (draw[0].astype(np.int64), draw[1], draw[2]), (draw[0][:-1], draw[1][:-1], draw[2][:-1]),
                (draw[0] + 3, draw[1], draw[2]), (draw[0], draw[1], draw[2].astype(np.float64))):
        with pytest.raises(ValueError, match="MixBank"):
            bank.mix(bad)


@pytest.mark.parametrize("N,hop,maxlen,target", [(64, 16, None, "mag"), (64, 16, 7, "mag"), (64, 16, None, "tpsa"),
                                                (64, 16, 7, "tpsa"), (512, 128, 7, "mag")])
def test_bank_tensors_are_wavs_to_tensors_of_the_mixtures(ops, bank, N, hop, maxlen, target):
    draw = bank.draw(snr_db=(-10.0, 20.0), seed=5, epoch=2)
    kw = dict(N=N, hop=hop, maxlen=maxlen, target=target)
    want = ops.wavs_to_tensors(bank.wavs(draw), bank.clean_wavs(), device=DEV, **kw)
    got = bank.tensors(draw, **kw)
    for a, b in zip(got, want):
        assert _same(a, b)
    if target == "mag":
        clean_only = ops.wavs_to_tensors(bank.clean_wavs(), bank.clean_wavs(), device=DEV, **kw)
        assert _same(got[1], clean_only[1]) and _same(got[2], clean_only[2]) and not _same(got[0], clean_only[0])
    # out=: the same tensors, rewritten in place with another draw, and back
    other = bank.draw(snr_db=(-10.0, 20.0), seed=5, epoch=3)
    first = tuple(t.clone() for t in got)
    ptrs = [t.data_ptr() for t in got]
    back = bank.tensors(other, out=got, **kw)
    assert all(a is b for a, b in zip(back, got)) and [t.data_ptr() for t in got] == ptrs
    assert not _same(got[0], first[0]) and _same(got[2], first[2])
    assert all(_same(a, b) for a, b in zip(got, ops.wavs_to_tensors(bank.wavs(other), bank.clean_wavs(), device=DEV,
                                                                    **kw)))
    bank.tensors(draw, out=got, **kw)
    assert all(_same(a, b) for a, b in zip(got, first))
    with pytest.raises(ValueError, match="out"):
        bank.tensors(draw, out=(got[0], got[1], got[2][:-1]), **kw)


def test_bank_frames_are_wavs_to_frames_of_the_mixtures(ops, bank):
    draw = bank.draw(snr_choices=[-5.0, 0.0, 5.0], seed=8)
    for N, hop in ((64, 16), (512, 128)):
        want = ops.wavs_to_frames(bank.wavs(draw), bank.clean_wavs(), N, hop)
        got = bank.frames(draw, N, hop)
        assert _same(got[0], want[0]) and _same(got[1], want[1])


# ---- training ----------------------------------------------------------------------------------------------
N_T, HOP_T, F_T, MAXLEN_T = 64, 16, 33, 20
SNR_T = (-5.0, 10.0)


def _model(family):
    from drnmf_amd import layers
    from oracle import drnmf_oracle as O
    torch.manual_seed(0)
    np.random.seed(0)
    if family == "snmf":
        r, K = 4, 2
        P = O.synth_problem(2, 4, F_T, r, seed=3)
        params = dict(input_dim=F_T, hidden_dim=2 * r, output_dim=F_T, mask_value=-1., maxseq=200, K_layers=K,
                      W=P["W"], alph=2 * r / 4.0, lam1=0.3, params_untied=["log_D", "log_alph"],
                      params_trainable=["log_D", "log_alph"])
        m = layers.build_unfolded_snmf(params, device=DEV)
    else:
        m = layers.build_lstm(dict(mask_value=-1., maxseq=200, input_dim=F_T, output_dim=F_T, K_layers=1,
                                   hidden_dim=8), device=DEV)
    m.compile(lr=1e-3)
    return m


class _Recorder(object):
    """A user callback: what the training tensors and the validation tensors hold when an epoch begins."""

    def __init__(self, seen):
        self.seen, self.x, self.val = seen, [], []

    def on_epoch_begin(self, ep, logs=None):
        self.x.append(tuple(t.clone() for t in (self.seen["x"], self.seen["y"], self.seen["w"])))
        self.val.append(tuple(t.clone() for t in self.seen["val"]))


def _fit_mixtures(family, seed, record=False):
    clean, noise = _recordings(33)
    clean_v, noise_v = _recordings(34, n_clean=3)
    from drnmf_amd import ops
    vb = ops.MixBank(clean_v, noise_v, device=DEV)
    validation = (vb.wavs(vb.draw(snr_db=SNR_T, seed=99)), vb.clean_wavs())
    m = _model(family)
    seen, inner = {}, m.fit

    def spy(x, y, **kw):                       # what fit_mixtures hands to fit
        seen.update(x=x, y=y, w=kw["sample_weight"], val=kw["validation_data"])
        return inner(x, y, **kw)
    m.fit = spy
    rec = _Recorder(seen)
    hist = m.fit_mixtures(clean, noise, snr_db=SNR_T, seed=seed, N=N_T, hop=HOP_T, maxlen=MAXLEN_T,
                          validation_wavs=validation, batch_size=4, epochs=3, shuffle_seed=123,
                          callbacks=[rec] if record else None)
    return m, hist, rec, validation


@pytest.mark.parametrize("family", ["snmf", "lstm"])
def test_fit_mixtures_draws_afresh_every_epoch(ops, family):
    clean, noise = _recordings(33)
    m, hist, rec, validation = _fit_mixtures(family, 1, record=True)
    bank = ops.MixBank(clean, noise, device=DEV)
    kw = dict(N=N_T, hop=HOP_T, maxlen=MAXLEN_T)
    assert len(rec.x) == 3
    for ep in range(3):
        want = bank.tensors(bank.draw(snr_db=SNR_T, seed=1, epoch=ep), **kw)
        assert all(_same(a, b) for a, b in zip(rec.x[ep], want)), ep
        assert all(_same(a, b) for a, b in zip(rec.val[ep], rec.val[0])), ep
    assert not _same(rec.x[0][0], rec.x[1][0]) and not _same(rec.x[1][0], rec.x[2][0])
    val = ops.wavs_to_tensors(validation[0], validation[1], device=DEV, **kw)
    assert all(_same(a, b) for a, b in zip(rec.val[0], val))
    for key in ("loss", "val_loss"):
        assert len(hist[key]) == 3 and np.all(np.isfinite(hist[key])) and np.all(np.array(hist[key]) > 0)
    # one seed, one result; another seed, another
    m2, hist2, _, _ = _fit_mixtures(family, 1)
    assert hist2 == hist
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    _, hist3, _, _ = _fit_mixtures(family, 2)
    assert hist3["loss"] != hist["loss"]
    # fit itself, driven by a callback of the test's that writes the same tensors
    x, y, w = bank.tensors(bank.draw(snr_db=SNR_T, seed=1, epoch=0), **kw)

    class Writer(object):
        def on_epoch_begin(self, ep, logs=None):
            for dst, src in zip((x, y, w), bank.tensors(bank.draw(snr_db=SNR_T, seed=1, epoch=ep), **kw)):
                dst.copy_(src)
    hist4 = _model(family).fit(x, y, sample_weight=w, validation_data=val, batch_size=4, epochs=3, seed=123,
                               callbacks=[Writer()])
    assert hist4 == hist


def test_from_mixtures_is_from_wavs_on_the_draw(ops):
    from drnmf_amd import layers
    clean, noise = _recordings(41)
    params = dict(r=4, sparsity=0.1, cf='ed', max_iter=5, conv_eps=0., random_seed=3)
    got = layers.SparseNMFModel.from_mixtures(clean, noise, params, snr_db=SNR_T, seed=4, N=N_T, hop=HOP_T, device=DEV)
    bank = ops.MixBank(clean, noise, device=DEV)
    want = layers.SparseNMFModel.from_wavs(bank.wavs(bank.draw(snr_db=SNR_T, seed=4)), bank.clean_wavs(), params, N=N_T,
                                           hop=HOP_T, device=DEV)
    for a, b in zip(got.get_weights(), want.get_weights()):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    other = layers.SparseNMFModel.from_mixtures(clean, noise, params, snr_db=SNR_T, seed=5, N=N_T, hop=HOP_T, device=DEV)
    assert not all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got.get_weights(), other.get_weights()))
    with pytest.raises(NotImplementedError, match="from_mixtures"):
        got.fit_mixtures(clean, noise)
