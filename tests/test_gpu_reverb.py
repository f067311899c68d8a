"""The device-side reverberator on the MI355X (include/drnmf_reverb.h): ops.reverb_forward against the fp64
reference of tests/reverb_ref.py at tile and chunk edges, every kind of delay and early count and both sample
types; exactly against an integer convolution; its degenerate rows; the bitwise independence of a signal from its
batch, stride and alignment path; ops.MixBank with RIRs against wavs_to_tensors / wavs_to_frames on the downloaded
mixtures and targets; fit_mixtures / from_mixtures with RIRs against fit / from_wavs on the same draws.

The bound (reverb_ref.BOUND) is 8 times the error of the float32 restatement of the header's chain on this file's
case list, measured on the host by tests/test_reverb_host.py, where every mutant of the reference misses it."""
import numpy as np
import pytest
import torch

import reverb_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _pack(rows, stride, fill):
    """[n][stride] with `fill` behind every row's length: values the kernel must never use."""
    out = np.full((len(rows), stride), fill, dtype=rows[0].dtype)
    for i, v in enumerate(rows):
        out[i, :len(v)] = v
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _guarded(n, stride, guard):
    """An [n][stride] float32 output filled with NaN inside a buffer with `guard` sentinels on either side."""
    buf = torch.full((2 * guard + n * stride,), -7.0, dtype=torch.float32, device=DEV)
    out = buf[guard:guard + n * stride].view(n, stride)
    out.fill_(float("nan"))
    return buf, out


def _run(ops, speech, lens, rirs, len_r, idx, delay, n_early, stride_s, stride_r=None, guard=3, want_early=True):
    """reverb_forward on packed rows: speech padded with a large value and RIRs with NaN behind their lengths,
    outputs pre-filled with NaN between guard columns.  Returns (wet, early) as numpy after checking the guards."""
    int16 = speech[0].dtype == np.int16
    sp = _dev(_pack(speech, stride_s, 30000 if int16 else 1e30))
    rr = _dev(_pack(rirs, stride_r or max(max(len(h) for h in rirs), 1), np.float32("nan")))
    n = len(speech)
    wbuf, wet = _guarded(n, stride_s, guard)
    ebuf, early = _guarded(n, stride_s, guard) if want_early else (None, None)
    got = ops.reverb_forward(sp, _dev(np.asarray(lens, dtype=np.int64)), rr, _dev(np.asarray(len_r, dtype=np.int64)),
                             _dev(np.asarray(idx, dtype=np.int32)),
                             delay=None if delay is None else _dev(np.asarray(delay, dtype=np.int32)),
                             n_early=None if n_early is None else _dev(np.asarray(n_early, dtype=np.int32)),
                             out=wet, early_out=early)
    assert (got[0] is wet and got[1] is early) if want_early else got is wet
    for buf in (wbuf, ebuf):
        if buf is not None:
            b = buf.cpu().numpy()
            assert (b[:guard] == -7.0).all() and (b[-guard:] == -7.0).all()           # nothing written outside
            assert not np.isnan(b).any()                                                # every element written
    return wet.cpu().numpy(), (early.cpu().numpy() if want_early else None)


def _run_batch(ops, b, stride_s, **kw):
    return _run(ops, b["speech"], b["lens"], b["rirs"], [len(h) for h in b["rirs"]], b["idx"], b["delay"], b["n_early"],
                stride_s, **kw)


def _tc(ops):
    return ops.REVERB_TILE, ops.REVERB_CHUNK


# ---- parity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sig,pad", [(1, 0), (5, 3), (70, 0), (70, 3)], ids=["1-odd", "5-aligned", "70-odd", "70-aligned"])
@pytest.mark.parametrize("int16", [True, False], ids=["int16", "float32"])
def test_reverb_matches_the_fp64_reference(ops, int16, n_sig, pad):
    T, C = _tc(ops)
    b = R.batch(n_sig, int16, T, C)
    stride = 2 * T + 5 + pad                       # 4101: odd; 4104: rows of aligned quads
    if n_sig == 70:
        assert set(b["lens"].tolist()) == set(R.speech_lens(T)) and len(set(b["idx"].tolist())) == 21
        L = np.array([len(h) for h in b["rirs"]])
        assert set(L.tolist()) == set(R.rir_lens(T, C)) and L.max() > b["lens"].max()
        assert set(zip((b["delay"] == 0).tolist(), (b["delay"] == L - 1).tolist())) >= {(True, False), (False, True),
                                                                                       (False, False)}
        assert {0, 1, C - 1, C} <= set(b["n_early"].tolist()) and (b["n_early"] == L).any() and (b["n_early"] > L).any()
    wet, early = _run_batch(ops, b, stride, guard=4 if pad else 3)      # 4 floats keep the rows' 16-byte alignment
    assert wet.shape == early.shape == (n_sig, stride) and wet.dtype == early.dtype == np.float32
    worst = 0.0
    for i, (ref_w, ref_e) in enumerate(b["ref"]):
        n = int(b["lens"][i])
        ew, ee = R.rel_err(wet[i, :n], ref_w), R.rel_err(early[i, :n], ref_e)
        worst = max(worst, ew, ee)
        assert ew <= R.BOUND and ee <= R.BOUND, (i, n, int(b["idx"][i]), ew, ee)
        assert not wet[i, n:].any() and not early[i, n:].any(), i                   # exactly 0 behind the length
        j = int(b["idx"][i])
        if b["n_early"][j] >= len(b["rirs"][j]):                                   # E == L: wet is early, bit for bit
            assert np.array_equal(_bits(wet[i]), _bits(early[i])), i
    print("worst error %.3g of max |reference| (bound %.3g)" % (worst, R.BOUND))


# ---- exact -------------------------------------------------------------------------------------------------
def test_reverb_is_the_integer_convolution_exactly(ops):
    """int16 samples within +-1024 and taps m / 256 with |m| <= 4: every product is an integer over 2^23 and every
    partial sum stays below 2^24 of them (1024 * 4 * 2051 < 2^24), so each chain, and the sum of the two parts,
    is exact in float32 in any order: the device must give the integer convolution, no tolerance."""
    T, C = _tc(ops)
    rng = np.random.default_rng(11)
    lens = R.speech_lens(T)
    rir_ints = [np.array([256]), np.array([128])] + [rng.integers(-4, 5, size=L) for L in (2, C - 1, C, C + 1, 2 * C + 3)]
    rirs = [(m / 256.0).astype(np.float32) for m in rir_ints]
    Ls = [len(m) for m in rir_ints]
    delay = [0, 0, 1, C // 2, C - 1, 0, 2 * C + 2]
    n_early = [1, 0, 1, C - 1, C, C, 2 * C + 3 + 5]
    n_sig = len(lens) * len(rirs)
    speech = [rng.integers(-1024, 1025, size=lens[i % 6]).astype(np.int16) for i in range(n_sig)]
    idx = np.arange(n_sig) // 6
    wet, early = _run(ops, speech, [len(s) for s in speech], rirs, Ls, idx, delay, n_early, 2 * T + 5)
    for i, s in enumerate(speech):
        j, n = int(idx[i]), len(s)
        d, E = R.clamp(delay[j], n_early[j], Ls[j])
        m = rir_ints[j].astype(np.int64)
        parts = []
        for a, bnd in ((0, E), (E, Ls[j])):
            c = np.convolve(s.astype(np.int64), m[a:bnd]) if bnd > a else np.zeros(1, np.int64)
            pos = np.arange(n) + d - a
            ok = (pos >= 0) & (pos < len(c))
            out = np.zeros(n, np.int64)
            out[ok] = c[pos[ok]]
            parts.append(out)
        want_e = (parts[0] / 2.0 ** 23).astype(np.float32)
        want_w = ((parts[0] + parts[1]) / 2.0 ** 23).astype(np.float32)
        assert np.abs(parts[0] + parts[1]).max() < 2 ** 24
        assert np.array_equal(wet[i, :n], want_w) and np.array_equal(early[i, :n], want_e), (i, j, n)
        assert not wet[i, n:].any() and not early[i, n:].any()
        if j == 0:                                  # h = [1]: wet is the speech, bit for bit
            assert np.array_equal(_bits(wet[i, :n]), _bits(s.astype(np.float32) / np.float32(32768.0)))
        if j == 1:                                  # h = [0.5], no early tap
            assert np.array_equal(wet[i, :n], s.astype(np.float32) / np.float32(65536.0)) and not early[i].any()


# ---- degenerate rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("int16", [True, False], ids=["int16", "float32"])
def test_rows_without_an_rir_are_the_speech_itself(ops, int16):
    T, C = _tc(ops)
    rng = np.random.default_rng(3)
    lens = [T + 1, 5, 2 * T + 5, 1, T]
    speech = [R.signal(rng, n, 0.1, int16) for n in lens]
    if not int16:
        speech[0][:3] = [-0.0, 1e-42, -1e-42]                          # a negative zero and denormals keep their bits
    # RIR 0: only NaN, and of length 0; RIR 1: NaN too, never indexed; RIR 2: a real one
    live = (0.5 * rng.standard_normal(40)).astype(np.float32)
    rirs = [np.full(40, np.nan, np.float32), np.full(40, np.nan, np.float32), live]
    len_r = [0, 40, 40]
    idx = [-1, 3, 0, -2 ** 31, 2]
    wet, early = _run(ops, speech, lens, rirs, len_r, idx, [5, 5, 5], [7, 7, 7], 2 * T + 5)
    assert np.isfinite(wet).all() and np.isfinite(early).all()
    for i in range(4):
        want = R.as_float(speech[i]).astype(np.float32)
        assert np.array_equal(_bits(wet[i, :lens[i]]), _bits(want)) and np.array_equal(_bits(early[i, :lens[i]]), _bits(want))
        assert not wet[i, lens[i]:].any() and not early[i, lens[i]:].any()
    ref_w, ref_e = R.reverb_one(speech[4], live, 5, 7)
    assert R.rel_err(wet[4, :T], ref_w) <= R.BOUND and R.rel_err(early[4, :T], ref_e) <= R.BOUND      # the rows are live
    assert not np.array_equal(wet[4, :T], R.as_float(speech[4]).astype(np.float32))


# ---- independence and coverage -----------------------------------------------------------------------------
@pytest.mark.parametrize("int16", [True, False], ids=["int16", "float32"])
def test_a_signal_does_not_depend_on_its_batch(ops, int16):
    T, C = _tc(ops)
    b = R.batch(70, int16, T, C)
    odd, aligned = 2 * T + 5, 2 * T + 8
    wet, early = _run_batch(ops, b, odd)                 # (_run: NaN pre-fill all overwritten, guards untouched)
    again = _run_batch(ops, b, odd)
    assert np.array_equal(_bits(again[0]), _bits(wet)) and np.array_equal(_bits(again[1]), _bits(early))
    # the aligned path (guard 4 keeps the 16-byte alignment), another RIR stride, and wet alone
    wide = _run_batch(ops, b, aligned, stride_r=6000, guard=4)
    assert np.array_equal(_bits(wide[0][:, :odd]), _bits(wet)) and np.array_equal(_bits(wide[1][:, :odd]), _bits(early))
    assert not wide[0][:, odd:].any() and not wide[1][:, odd:].any()
    alone = _run_batch(ops, b, aligned, guard=4, want_early=False)
    assert alone[1] is None and np.array_equal(_bits(alone[0]), _bits(wide[0]))
    # one signal of every length alone, at its own stride, with its RIR alone in the bank
    for i in (0, 1, 2, 3, 4, 5, 26, 47, 69):
        j, n = int(b["idx"][i]), int(b["lens"][i])
        for stride in (n, n + (-n) % 4 + 4):
            one = _run(ops, [b["speech"][i]], [n], [b["rirs"][j]], [len(b["rirs"][j])], [0], [b["delay"][j]],
                       [b["n_early"][j]], stride, guard=4 if stride % 4 == 0 else 3)
            assert np.array_equal(_bits(one[0][0, :n]), _bits(wet[i, :n])), (i, stride)
            assert np.array_equal(_bits(one[1][0, :n]), _bits(early[i, :n])), (i, stride)
    # another batch position
    perm = np.roll(np.arange(70), 17)
    moved = dict(b, speech=[b["speech"][p] for p in perm], lens=b["lens"][perm], idx=b["idx"][perm])
    got = _run_batch(ops, moved, odd)
    assert np.array_equal(_bits(got[0]), _bits(wet[perm])) and np.array_equal(_bits(got[1]), _bits(early[perm]))
    # no early counts: E == L for every RIR, and wet is early bit for bit; no delays: d = 0
    full = _run(ops, b["speech"], b["lens"], b["rirs"], [len(h) for h in b["rirs"]], b["idx"], b["delay"], None, odd)
    assert np.array_equal(_bits(full[0]), _bits(full[1]))
    causal = _run(ops, b["speech"], b["lens"], b["rirs"], [len(h) for h in b["rirs"]], b["idx"], None, None, odd)
    for i in (5, 11, 40):
        ref = R.reverb_one(b["speech"][i], b["rirs"][b["idx"][i]])[0]
        assert R.rel_err(causal[0][i, :len(ref)], ref) <= R.BOUND, i


def test_more_than_65535_signals(ops):
    """The launch is cut into slices of 65 535 rows: 70 000 short signals, seven distinct ones repeated, give the
    bits of the first seven everywhere, and those are the reference's."""
    rng = np.random.default_rng(8)
    n_sig, period, stride = 70000, 7, 9
    speech = [R.signal(rng, n, 0.1, False) for n in (9, 1, 5, 8, 2, 7, 3)]
    rirs = [(0.5 * rng.standard_normal(L)).astype(np.float32) for L in (4, 11)]
    idx = np.arange(period) % 2
    reps = n_sig // period
    tile = lambda a: np.tile(a, (reps,) + (1,) * (np.ndim(a) - 1))
    lens = np.array([len(v) for v in speech])
    wet, early = _run(ops, speech * reps, tile(lens), rirs, [4, 11], tile(idx), [1, 3], [2, 20], stride)
    assert np.array_equal(_bits(wet), _bits(tile(wet[:period]))) and np.array_equal(_bits(early), _bits(tile(early[:period])))
    for i in range(period):
        ref = R.reverb_one(speech[i], rirs[idx[i]], [1, 3][idx[i]], [2, 20][idx[i]])
        assert R.rel_err(wet[i, :lens[i]], ref[0]) <= R.BOUND and R.rel_err(early[i, :lens[i]], ref[1]) <= R.BOUND


# ---- the bank ----------------------------------------------------------------------------------------------
def _recordings(seed, n_clean=6, int16=True):
    rng = np.random.default_rng(seed)
    lens = rng.integers(300, 1500, size=n_clean)
    lens[0], lens[1] = 1499, 37                                             # an odd stride; shorter than one window
    clean = [R.signal(rng, int(n), 0.1, int16) for n in lens]
    noise = [R.signal(rng, int(n), 0.05, not int16) for n in (2000, 333, 5)]
    return clean, noise


def _rirs(ops):
    """Three stand-in RIRs of 160 to 1280 taps; the second with its direct path at tap 9, the third longer than
    most utterances."""
    a, b, c = ops.synthetic_rirs(3, fs=16000, rt60=(0.01, 0.08), seed=2)
    b = np.concatenate([0.01 * np.ones(9, np.float32), b])
    return [a, b, c]


_banks = {}


def _bank(ops, target_speech, align=True):
    key = (target_speech, align)
    if key not in _banks:
        clean, noise = _recordings(21)
        _banks[key] = ops.MixBank(clean, noise, rirs=_rirs(ops), target_speech=target_speech, align=align, early_ms=5.0,
                                  device=DEV)
    return _banks[key]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32),
                                                                                       b.view(torch.int32))


def test_bank_reverberates_then_mixes(ops):
    clean, noise = _recordings(21)
    rirs = _rirs(ops)
    bank = _bank(ops, 'early')
    assert ops.rir_delays(rirs).tolist() == [0, 9, 0] and bank.rir_delay.tolist() == [0, 9, 0]
    assert bank.rir_n_early.tolist() == [81, 90, 81]                       # delay + 1 + round(5 ms * 16 kHz)
    draw = bank.draw(snr_db=(-10.0, 20.0), seed=7, epoch=1, reverb_prob=0.7)
    assert len(draw) == 4 and set(draw[3].tolist()) == {-1, 0, 1, 2}        # every RIR, and dry utterances
    noisy, early = bank.wavs(draw), bank.target_wavs(draw)
    wet = _bank(ops, 'reverberant').target_wavs(draw)
    dry = _bank(ops, 'dry').target_wavs(draw)
    worst = 0.0
    for i, s in enumerate(clean):
        j = int(draw[3][i])
        h = rirs[j] if j >= 0 else None
        ref_w, ref_e = R.reverb_one(s, h, None if h is None else int(bank.rir_delay[j]),
                                    None if h is None else int(bank.rir_n_early[j]))
        assert R.rel_err(wet[i], ref_w) <= R.BOUND and R.rel_err(early[i], ref_e) <= R.BOUND, i
        assert np.array_equal(dry[i], R.as_float(s).astype(np.float32))
        if j < 0:
            assert np.array_equal(_bits(wet[i]), _bits(dry[i])) and np.array_equal(_bits(early[i]), _bits(dry[i]))
        # the SNR of the request is that of the reverberant speech in the mixture
        d = abs(_realised_snr_db(wet[i].astype(np.float64), noisy[i].astype(np.float64)) - float(draw[2][i]))
        worst = max(worst, d)
        assert d <= 1e-3, (i, d)
    print("realised SNR of the wet speech within %.3g dB" % worst)
    # align=False: the causal convolution, delays 0; 'dry' then has no aligned target
    causal = _bank(ops, 'reverberant', align=False)
    assert causal.rir_delay.tolist() == [0, 0, 0] and causal.rir_n_early.tolist() == [81, 81, 81]
    cw = causal.target_wavs(draw)
    for i, s in enumerate(clean):
        j = int(draw[3][i])
        if j >= 0:
            assert R.rel_err(cw[i], R.reverb_one(s, rirs[j])[0]) <= R.BOUND, i
    with pytest.raises(ValueError, match="align"):
        ops.MixBank(clean, noise, rirs=rirs, target_speech='dry', align=False, device=DEV)
    # a draw of the other arity, and an RIR index outside the bank, are refused
    for bad in (draw[:3], draw[:3] + (draw[3] + 3,), draw[:3] + (draw[3].astype(np.int64),)):
        with pytest.raises(ValueError, match="MixBank"):
            bank.mix(bad)


def _realised_snr_db(speech, noisy):
    d = noisy - speech
    return 10.0 * np.log10(np.sum(speech * speech) / np.sum(d * d))


@pytest.mark.parametrize("target", ["mag", "tpsa"])
@pytest.mark.parametrize("target_speech", ["reverberant", "early", "dry"])
def test_bank_tensors_and_frames_are_those_of_the_downloaded_pairs(ops, target_speech, target):
    bank = _bank(ops, target_speech)
    draw = bank.draw(snr_db=(-10.0, 20.0), seed=5, epoch=2, reverb_prob=0.8)
    kw = dict(N=64, hop=16, maxlen=7, target=target)
    pairs = (bank.wavs(draw), bank.target_wavs(draw))
    want = ops.wavs_to_tensors(*pairs, device=DEV, **kw)
    got = bank.tensors(draw, **kw)
    assert all(_same(a, b) for a, b in zip(got, want))
    # out=: rewritten in place with another draw, and back
    other = bank.draw(snr_db=(-10.0, 20.0), seed=5, epoch=3, reverb_prob=0.8)
    first = tuple(t.clone() for t in got)
    back = bank.tensors(other, out=got, **kw)
    assert all(a is b for a, b in zip(back, got)) and not _same(got[0], first[0]) and _same(got[2], first[2])
    assert _same(got[1], first[1]) == (target_speech == 'dry' and target == 'mag')     # the target moves with the RIRs
    bank.tensors(draw, out=got, **kw)
    assert all(_same(a, b) for a, b in zip(got, first))
    if target == "mag":
        wf = ops.wavs_to_frames(*pairs, 64, 16)
        gf = bank.frames(draw, 64, 16)
        assert _same(gf[0], wf[0]) and _same(gf[1], wf[1])


def test_a_bank_without_rirs_is_the_bank_of_before(ops):
    clean, noise = _recordings(21)
    plain = ops.MixBank(clean, noise, device=DEV)
    assert plain.n_rir == 0 and not hasattr(plain, "wet")
    draw = plain.draw(snr_db=(-10.0, 20.0), seed=5, epoch=2)
    assert len(draw) == 3
    kw = dict(N=64, hop=16, maxlen=7)
    got = plain.tensors(draw, **kw)
    want = ops.wavs_to_tensors(plain.wavs(draw), plain.clean_wavs(), device=DEV, **kw)
    assert all(_same(a, b) for a, b in zip(got, want))
    assert all(np.array_equal(a, b) for a, b in zip(plain.target_wavs(draw), plain.clean_wavs()))
    # the mixtures are mix_forward's on the clean side with the energies the bank keeps
    idx, off, snr = draw
    direct = ops.mix_forward(plain.clean, plain.len_clean_dev, plain.noise, plain.len_noise_dev, _dev(idx), _dev(off),
                             _dev(snr), speech_energy=plain.energy)
    assert _same(direct, plain.mix(draw)[0])
    with pytest.raises(ValueError, match="MixBank"):
        plain.mix(draw + (np.zeros(len(clean), np.int32),))
    # and a bank with RIRs whose draw leaves every utterance dry gives the same tensors, bit for bit
    wet = _bank(ops, 'reverberant')
    dry_draw = wet.draw(snr_db=(-10.0, 20.0), seed=5, epoch=2, reverb_prob=0.0)
    assert all(np.array_equal(a, b) for a, b in zip(dry_draw[:3], draw)) and (dry_draw[3] == -1).all()
    assert all(_same(a, b) for a, b in zip(wet.tensors(dry_draw, **kw), got))


# ---- training ----------------------------------------------------------------------------------------------
N_T, HOP_T, F_T, MAXLEN_T = 64, 16, 33, 20
SNR_T = (-5.0, 10.0)
REVERB_T = dict(reverb_prob=0.7, target_speech='early', early_ms=5.0)


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


def _fit_mixtures(ops, family, seed):
    clean, noise = _recordings(33)
    m = _model(family)
    hist = m.fit_mixtures(clean, noise, snr_db=SNR_T, seed=seed, N=N_T, hop=HOP_T, maxlen=MAXLEN_T, rirs=_rirs(ops),
                          batch_size=4, epochs=2, shuffle_seed=123, **REVERB_T)
    return m, hist


@pytest.mark.parametrize("family", ["snmf", "lstm"])
def test_fit_mixtures_with_rirs_is_fit_on_the_same_draws(ops, family):
    clean, noise = _recordings(33)
    m, hist = _fit_mixtures(ops, family, 1)
    assert len(hist["loss"]) == 2 and np.all(np.isfinite(hist["loss"])) and np.all(np.array(hist["loss"]) > 0)
    m2, hist2 = _fit_mixtures(ops, family, 1)
    assert hist2 == hist
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    # fit itself, driven by a callback of the test's that writes the same tensors
    bank = ops.MixBank(clean, noise, rirs=_rirs(ops), target_speech='early', early_ms=5.0, device=DEV)
    kw = dict(N=N_T, hop=HOP_T, maxlen=MAXLEN_T)
    draws = [bank.draw(snr_db=SNR_T, seed=1, epoch=ep, reverb_prob=0.7) for ep in range(2)]
    assert not np.array_equal(draws[0][3], draws[1][3])                    # another RIR table every epoch
    assert all((d[3] == -1).any() and (d[3] >= 0).any() for d in draws)
    x, y, w = bank.tensors(draws[0], **kw)

    class Writer(object):
        def on_epoch_begin(self, ep, logs=None):
            for dst, src in zip((x, y, w), bank.tensors(draws[ep], **kw)):
                dst.copy_(src)
    hist3 = _model(family).fit(x, y, sample_weight=w, batch_size=4, epochs=2, seed=123, callbacks=[Writer()])
    assert hist3 == hist
    # the RIRs matter: without them another result
    plain = _model(family).fit_mixtures(clean, noise, snr_db=SNR_T, seed=1, N=N_T, hop=HOP_T, maxlen=MAXLEN_T,
                                        batch_size=4, epochs=2, shuffle_seed=123)
    assert plain["loss"] != hist["loss"]


def test_from_mixtures_with_rirs_is_from_wavs_on_the_draw(ops):
    from drnmf_amd import layers
    clean, noise = _recordings(41)
    params = dict(r=4, sparsity=0.1, cf='ed', max_iter=5, conv_eps=0., random_seed=3)
    got = layers.SparseNMFModel.from_mixtures(clean, noise, params, snr_db=SNR_T, seed=4, N=N_T, hop=HOP_T, device=DEV,
                                              rirs=_rirs(ops), reverb_prob=0.7)
    bank = ops.MixBank(clean, noise, rirs=_rirs(ops), device=DEV)
    draw = bank.draw(snr_db=SNR_T, seed=4, reverb_prob=0.7)
    want = layers.SparseNMFModel.from_wavs(bank.wavs(draw), bank.target_wavs(draw), params, N=N_T, hop=HOP_T, device=DEV)
    for a, b in zip(got.get_weights(), want.get_weights()):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    plain = layers.SparseNMFModel.from_mixtures(clean, noise, params, snr_db=SNR_T, seed=4, N=N_T, hop=HOP_T, device=DEV)
    assert not all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got.get_weights(), plain.get_weights()))
