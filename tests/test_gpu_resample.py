"""The device-side resampler on the MI355X (include/drnmf_resample.h) against tests/resample_ref.py: every rate pair
at the kernel's edge lengths, both input types, padding and guards, batch invariance, the chunked form's bits, and
the two users, ops.MixBank(clean_fs=, noise_fs=, rir_fs=) and model.enhance(fs_in=).

Tolerance.  |out - ref| <= 2^-24 |ref| + 1e-12 max|x|: the one float32 rounding, plus the fp64 chain's reordering
and the device's Bessel / sinpi against numpy's -- a few hundred terms of 2^-53 sum|h| max|x|, orders below 1e-12."""
import numpy as np
import pytest
import torch

import resample_ref as R
from oracle import drnmf_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAIRS = [pytest.param(*r, id="%d-%d" % r[:2]) for r in R.RATE_PAIRS]
STREAM_PAIRS = [pytest.param(*r, id="%d-%d" % r[:2]) for r in R.RATE_PAIRS[:3]]      # 1/3, 2/1, 160/441


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _signal(n, seed, int16):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal(n) * (1.0 + 0.5 * np.sin(np.arange(n) / 37.0))
    return (x * 6000).astype(np.int16) if int16 else (0.25 * x).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _close(got, x, p, q, what):
    """got (float32) against the reference of x within the tolerance of the module's docstring."""
    ref = R.resample(x, p, q)
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.shape[0] == 0:
        return
    xmax = np.abs(R.as_samples(x)).max() if len(x) else 0.0
    err = np.abs(got.astype(np.float64) - ref)
    bound = 2.0 ** -24 * np.abs(ref) + 1e-12 * xmax
    worst = int(np.argmax(err - bound))
    assert (err <= bound).all(), (what, worst, err[worst], bound[worst])


def _edge_lengths(ops, fs_in, fs_out, p, q):
    """0, 1, 2 samples; one fewer than half / p + 1 (shorter than half the filter); output counts of tile - 1, tile,
    tile + 1 and 2 tile + 1 (the largest count not above the target where p > q cannot hit it)."""
    tile = ops.resample_tile(fs_in, fs_out)
    assert tile == ops.RESAMPLE_TILE
    half = 0 if p == q else 10 * max(p, q)
    lens = [0, 1, 2, max(half // p, 3)]
    for target in (tile - 1, tile, tile + 1, 2 * tile + 1):
        n = target * q // p
        assert R.out_len(n, p, q) <= target and (p > q or R.out_len(n, p, q) == target)
        lens.append(n)
    return lens


@pytest.mark.parametrize("int16", [True, False], ids=["int16", "float32"])
@pytest.mark.parametrize("fs_in,fs_out,p,q", PAIRS)
def test_rate_pairs_at_the_edge_lengths(ops, fs_in, fs_out, p, q, int16):
    lens = _edge_lengths(ops, fs_in, fs_out, p, q)
    xs = [_signal(n, 100 + i, int16) for i, n in enumerate(lens)]
    y, n_out = ops.resample(xs, fs_in, fs_out, device=DEV)
    assert y.dtype == torch.float32 and y.device == torch.device(DEV)
    assert n_out.dtype == np.int64 and n_out.tolist() == [R.out_len(n, p, q) for n in lens]
    assert tuple(y.shape) == (len(lens), max(1, int(n_out.max())))
    assert ops.resample_out_lengths(lens, fs_in, fs_out).tolist() == n_out.tolist()
    yh = y.cpu().numpy()
    for i, x in enumerate(xs):
        k = int(n_out[i])
        _close(yh[i, :k], x, p, q, (lens[i], int16))
        assert not yh[i, k:].any() and not np.signbit(yh[i, k:]).any(), lens[i]        # 0.0f behind the length
        if p == q:      # the copy is exact
            assert np.array_equal(_bits(yh[i, :k]), _bits(R.as_samples(x).astype(np.float32)))
    wavs = ops.resample_wavs(xs, fs_in, fs_out, device=DEV)
    for i, w in enumerate(wavs):
        assert w.dtype == np.float32 and np.array_equal(_bits(w), _bits(yh[i, :int(n_out[i])]))


def _ragged(ops, fs_in, fs_out, int16):
    """Three rows (1, 701 and 2 tile + 1 samples) in a device buffer with odd strides and a base one element off,
    NaN (float32) or junk (int16) behind every row's length, guard elements around the output."""
    tile = ops.resample_tile(fs_in, fs_out)
    lens = [1, 701, 2 * tile + 1]
    xs = [_signal(n, 7 + i, int16) for i, n in enumerate(lens)]
    si = max(lens) + 2
    si += 1 - si % 2
    host = np.full(1 + 3 * si, 12345 if int16 else np.nan, dtype=np.int16 if int16 else np.float32)
    rows = host[1:].reshape(3, si)
    for i, x in enumerate(xs):
        rows[i, :len(x)] = x
    buf = torch.from_numpy(host).to(DEV)
    x = buf[1:].view(3, si)
    assert x.data_ptr() % 4 == (2 if int16 else 0) and x.data_ptr() % 16 != 0 and si % 2 == 1
    return xs, lens, x


@pytest.mark.parametrize("int16", [True, False], ids=["int16", "float32"])
@pytest.mark.parametrize("fs_in,fs_out,p,q", PAIRS)
def test_ragged_batch_padding_guards_and_batch_invariance(ops, fs_in, fs_out, p, q, int16):
    xs, lens, x = _ragged(ops, fs_in, fs_out, int16)
    n_want = [R.out_len(n, p, q) for n in lens]
    so = max(n_want) + 4
    so += 1 - so % 2
    guard = torch.full((1 + 3 * so + 5,), 7.5, dtype=torch.float32, device=DEV)
    out = guard[1:1 + 3 * so].view(3, so)
    y, n_out = ops.resample(x, fs_in, fs_out, lengths=lens, out=out)
    assert y is out and n_out.tolist() == n_want
    g = guard.cpu().numpy()
    assert g[0] == 7.5 and (g[1 + 3 * so:] == 7.5).all()                # nothing outside out
    yh = g[1:1 + 3 * so].reshape(3, so)
    for i in range(3):
        k = n_want[i]
        _close(yh[i, :k].copy(), xs[i], p, q, (lens[i], int16))
        assert _bits(yh[i, k:]).max() == 0, lens[i]                      # every element behind the length is +0.0f
        alone = ops.resample_wavs([xs[i]], fs_in, fs_out, device=DEV)[0]
        assert np.array_equal(_bits(alone), _bits(yh[i, :k])), lens[i]   # the row's bits do not depend on its batch
    # lengths on the device clamp to the row; a 2-D host array is the same call
    yb, _ = ops.resample(x.cpu().numpy(), fs_in, fs_out, lengths=lens, device=DEV)
    for i in range(3):
        assert np.array_equal(_bits(yb[i, :n_want[i]].cpu().numpy()), _bits(yh[i, :n_want[i]]))


@pytest.mark.parametrize("fs_out,q,n", [(800, 20, 40000), (25, 640, 3000)])
def test_steep_decimation_shrinks_the_tile(ops, fs_out, q, n):
    """Where the input span of 2048 outputs does not fit beside the table in LDS a tile is fewer outputs: 1988 at
    1 / 20, and 4 at 1 / 640, whose table and span take all 160 KiB of a compute unit.  More than one tile each."""
    tile = ops.resample_tile(16000, fs_out)
    assert ops.resample_rate(16000, fs_out) == (1, q) and tile == {20: 1988, 640: 4}[q]
    xs = [_signal(n, 3, False), _signal(n // 2 + 1, 4, False)]
    wavs = ops.resample_wavs(xs, 16000, fs_out, device=DEV)
    assert len(wavs[0]) == R.out_len(n, 1, q) > tile
    for w, x in zip(wavs, xs):
        _close(w, x, 1, q, (q, len(x)))


def _stream_lengths(ops, fs_in, fs_out, p, q):
    big = ops.resample_tile(fs_in, fs_out) * q // p + 50      # a chunk that gives more than a tile of outputs
    return big, dict(ones=(40, 97, 150), zeros=(50, 120, 200), big=(big + 10, big + 500, 9), random=(1000, 2500, 1777))


@pytest.mark.parametrize("chunking,int16", [("ones", False), ("zeros", False), ("big", False), ("random", False),
                                            ("random", True)])
@pytest.mark.parametrize("fs_in,fs_out,p,q", STREAM_PAIRS)
def test_chunked_form_has_the_offline_bits(ops, fs_in, fs_out, p, q, chunking, int16):
    big, table = _stream_lengths(ops, fs_in, fs_out, p, q)
    lens = table[chunking]
    xs = [_signal(n, 40 + i, int16) for i, n in enumerate(lens)]
    cuts = [R.chunkings(n, seed=n, big=big)[chunking] for n in lens]
    want = ops.resample_wavs(xs, fs_in, fs_out, device=DEV)
    st = ops.ResampleStream(3, fs_in, fs_out, dtype='int16' if int16 else 'float32', device=DEV)
    empty = np.zeros(0, dtype=xs[0].dtype)
    for attempt in range(2):
        got = [[] for _ in lens]
        for j in range(max(len(c) for c in cuts) - 1):
            chunks = [x[c[j]:c[j + 1]] if j + 1 < len(c) else empty for x, c in zip(xs, cuts)]
            for i, piece in enumerate(st.push(chunks)):
                assert piece.dtype == np.float32
                got[i].append(piece)
        for i, piece in enumerate(st.close()):
            got[i].append(piece)
        with pytest.raises(ValueError):
            st.push([empty] * 3)
        for i, n in enumerate(lens):
            y = np.concatenate(got[i])
            assert y.shape[0] == R.out_len(n, p, q) == want[i].shape[0], (attempt, n)
            assert np.array_equal(_bits(y), _bits(want[i])), (attempt, n)
        st.reset()


def test_chunked_copy_and_argument_checks_of_the_stream(ops):
    x = _signal(300, 1, False)
    st = ops.ResampleStream(1, 16000, 16000, device=DEV)
    got = [st.push([x[:7]])[0], st.push([x[7:7]])[0], st.push([x[7:]])[0], st.close()[0]]
    assert [len(g) for g in got] == [7, 0, 293, 0] and np.array_equal(_bits(np.concatenate(got)), _bits(x))
    for bad in (dict(n_streams=0), dict(dtype='float64'), dict(fs_in=0), dict(fs_out=44101)):
        kw = dict(n_streams=2, fs_in=16000, fs_out=8000, dtype='float32', device=DEV)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.ResampleStream(**kw)
    st = ops.ResampleStream(2, 48000, 16000, device=DEV)
    for chunks in ([x], [x, x.astype(np.float64)], [x, x.reshape(2, -1)], [x, (x * 100).astype(np.int16)]):
        with pytest.raises(ValueError):
            st.push(chunks)


def test_argument_checks(ops):
    f, i = _signal(100, 1, False), _signal(100, 2, True)
    x = torch.zeros((2, 50), dtype=torch.float32, device=DEV)
    for call in (lambda: ops.resample([f, i], 48000, 16000, device=DEV),                 # mixed types
                 lambda: ops.resample([f, f.astype(np.float64)], 48000, 16000, device=DEV),
                 lambda: ops.resample([f.reshape(2, 50)[0:1]], 48000, 16000, device=DEV),
                 lambda: ops.resample([], 48000, 16000, device=DEV),
                 lambda: ops.resample([f], 48000, 16000, lengths=[100], device=DEV),     # lengths with a list
                 lambda: ops.resample(x, 48000, 16000),                                  # no lengths
                 lambda: ops.resample(x, 48000, 16000, lengths=[50, 51]),                # beyond the row width
                 lambda: ops.resample(x, 48000, 16000, lengths=[50, -1]),
                 lambda: ops.resample(x, 48000, 16000, lengths=[50]),
                 lambda: ops.resample(x.cpu(), 48000, 16000, lengths=[50, 50]),          # not on the device
                 lambda: ops.resample(x.double(), 48000, 16000, lengths=[50, 50]),
                 lambda: ops.resample(x, 48000, 16000, lengths=[50, 50],                 # out: too narrow
                                      out=torch.zeros((2, 16), dtype=torch.float32, device=DEV)),
                 lambda: ops.resample(x, 48000, 16000, lengths=[50, 50],                 # out: rows
                                      out=torch.zeros((3, 17), dtype=torch.float32, device=DEV)),
                 lambda: ops.resample(x, 48000, 16000, lengths=[50, 50],                 # out: type
                                      out=torch.zeros((2, 17), dtype=torch.float64, device=DEV)),
                 lambda: ops.resample(x, 48000, 16000, lengths=[50, 50],                 # out: device
                                      out=torch.zeros((2, 17), dtype=torch.float32)),
                 lambda: ops.resample(x, 48000, 16000, lengths=[50, 50],                 # out: not contiguous
                                      out=torch.zeros((2, 34), dtype=torch.float32, device=DEV)[:, ::2]),
                 lambda: ops.resample(x, 0, 16000, lengths=[50, 50]),
                 lambda: ops.resample(x, 16000, 44101, lengths=[50, 50]),
                 lambda: ops.resample(x, 48000, 16000, lengths=[50, 50], nz=0),
                 lambda: ops.resample(x, 48000, 16000, lengths=[50, 50], beta=-1.0)):
        with pytest.raises(ValueError):
            call()
    y, n = ops.resample(x, 48000, 16000, lengths=[50, 50], out=torch.ones((2, 17), dtype=torch.float32, device=DEV))
    assert n.tolist() == [17, 17] and not y.cpu().numpy().any()
    y, n = ops.resample([i[:0], i[:0]], 48000, 16000, device=DEV)                           # nothing at all
    assert n.tolist() == [0, 0] and tuple(y.shape) == (2, 1) and not y.cpu().numpy().any()
    # other filters than the default follow the same definition
    y = ops.resample_wavs([f], 48000, 16000, nz=4, beta=8.0, device=DEV)[0]
    ref = R.resample(f, 1, 3, nz=4, beta=8.0)
    assert np.abs(y - ref).max() <= 2.0 ** -24 * np.abs(ref).max() + 1e-12


# ---- the banks ------------------------------------------------------------------------------------------------
N_B, HOP_B = 64, 16


def _recordings(seed=5):
    rs = np.random.RandomState(seed)
    clean = [(rs.standard_normal(n) * 4000).astype(np.int16) for n in (900, 1301, 640, 1111)]
    noise = [(0.1 * rs.standard_normal(n)).astype(np.float32) for n in (7000, 5003)]
    return clean, noise


def _same_draw(ops, a, b):
    """One draw through both banks: equal lengths, energies and bits of tensors(...)."""
    assert np.array_equal(a.len_clean, b.len_clean) and np.array_equal(a.len_noise, b.len_noise)
    assert a.n == b.n and a.n_noise == b.n_noise and a.n_rir == b.n_rir
    draw = a.draw(snr_db=(-3.0, 6.0), seed=11, epoch=2)
    for u, v in zip(draw, b.draw(snr_db=(-3.0, 6.0), seed=11, epoch=2)):
        assert np.array_equal(u, v)
    ta, tb = a.tensors(draw, N=N_B, hop=HOP_B), b.tensors(draw, N=N_B, hop=HOP_B)
    for u, v in zip(ta, tb):
        assert u.shape == v.shape and torch.equal(u.view(torch.int32), v.view(torch.int32))
    for u, v in zip(a.wavs(draw), b.wavs(draw)):
        assert np.array_equal(_bits(u), _bits(v))
    if a.energy is not None:
        assert torch.equal(a.energy, b.energy)


def test_mixbank_noise_side_at_another_rate(ops):
    clean, noise = _recordings()
    noise48 = [(0.1 * np.random.RandomState(i).standard_normal(n)).astype(np.float32) for i, n in enumerate((21000, 15010))]
    a = ops.MixBank(clean, noise48, noise_fs=48000, device=DEV)
    b = ops.MixBank(clean, ops.resample_wavs(noise48, 48000, 16000, device=DEV), device=DEV)
    assert a.noise.dtype == torch.float32 and a.len_noise.tolist() == [7000, 5004]
    _same_draw(ops, a, b)
    i16 = [(w * 30000).astype(np.int16) for w in noise48]
    a = ops.MixBank(clean, i16, noise_fs=48000, device=DEV)
    assert a.noise.dtype == torch.float32                       # a resampled noise side is held as float32
    _same_draw(ops, a, ops.MixBank(clean, ops.resample_wavs(i16, 48000, 16000, device=DEV), device=DEV))


def test_mixbank_clean_and_rir_sides_at_other_rates(ops):
    clean, noise = _recordings()
    clean8 = [w[:len(w) // 2].copy() for w in clean]
    a = ops.MixBank(clean8, noise, clean_fs=8000, device=DEV)
    b = ops.MixBank(ops.resample_wavs(clean8, 8000, 16000, device=DEV), noise, device=DEV)
    _same_draw(ops, a, b)
    rirs48 = ops.synthetic_rirs(3, fs=48000, rt60=(0.01, 0.03), seed=2)
    for kw in (dict(), dict(align=False), dict(target_speech='early', early_ms=5.0)):
        a = ops.MixBank(clean, noise, rirs=rirs48, rir_fs=48000, device=DEV, **kw)
        b = ops.MixBank(clean, noise, rirs=ops.resample_wavs(rirs48, 48000, 16000, device=DEV), device=DEV, **kw)
        assert torch.equal(a.rir_delay, b.rir_delay) and torch.equal(a.rir_n_early, b.rir_n_early)
        _same_draw(ops, a, b)


def test_mixbank_without_side_rates_is_the_bank_of_before(ops):
    clean, noise = _recordings()
    rirs = ops.synthetic_rirs(3, fs=16000, rt60=(0.01, 0.03), seed=2)
    for kw in (dict(), dict(rirs=rirs)):
        a = ops.MixBank(clean, noise, device=DEV, **kw)
        b = ops.MixBank(clean, noise, device=DEV, clean_fs=None, noise_fs=None, rir_fs=None, **kw)
        c = ops.MixBank(clean, noise, device=DEV, clean_fs=16000, noise_fs=16000.0, rir_fs=16000, **kw)
        assert a.clean.dtype == c.clean.dtype == torch.float32 and c.noise.dtype == a.noise.dtype
        _same_draw(ops, a, b)
        _same_draw(ops, a, c)
    for kw in (dict(clean_fs=0), dict(noise_fs=44101), dict(rirs=rirs, rir_fs=-1), dict(noise_fs=16000.5)):
        with pytest.raises(ValueError):
            ops.MixBank(clean, noise, device=DEV, **kw)
    a = ops.MixBank(clean, noise, device=DEV, rir_fs=48000)         # no RIRs: their rate is not looked at
    _same_draw(ops, a, ops.MixBank(clean, noise, device=DEV))


def test_fit_mixtures_and_from_mixtures_pass_the_side_rates_on(ops):
    """Both calls with noise_fs=48000 train as on the noise resampled beforehand: same history, same weights."""
    from drnmf_amd import layers
    clean, _ = _recordings()
    noise48 = [(0.1 * np.random.RandomState(i).standard_normal(n)).astype(np.float32) for i, n in enumerate((21000, 15010))]
    noise16 = ops.resample_wavs(noise48, 48000, 16000, device=DEV)

    def fit(noise, **kw):
        torch.manual_seed(0)
        np.random.seed(0)
        m = layers.build_lstm(dict(mask_value=-1., maxseq=200, input_dim=F_E, output_dim=F_E, K_layers=1,
                                   hidden_dim=8), device=DEV)
        m.compile(lr=1e-3)
        return m, m.fit_mixtures(clean, noise, snr_db=(0.0, 6.0), seed=2, N=N_B, hop=HOP_B, maxlen=40, batch_size=4,
                                 epochs=2, shuffle_seed=5, **kw)
    (ma, ha), (mb, hb) = fit(noise48, noise_fs=48000), fit(noise16)
    assert ha == hb and len(ha["loss"]) == 2 and np.all(np.isfinite(ha["loss"]))
    for u, v in zip(ma.get_weights(), mb.get_weights()):
        assert np.array_equal(np.asarray(u), np.asarray(v))
    with pytest.raises(ValueError):
        fit(noise48, noise_fs=44101)
    params = dict(r=4, sparsity=0.1, cf='ed', max_iter=5, conv_eps=0., random_seed=3)
    kw = dict(snr_db=(0.0, 6.0), seed=4, N=N_B, hop=HOP_B, device=DEV)
    got = layers.SparseNMFModel.from_mixtures(clean, noise48, params, noise_fs=48000, **kw)
    want = layers.SparseNMFModel.from_mixtures(clean, noise16, params, **kw)
    for u, v in zip(got.get_weights(), want.get_weights()):
        assert np.array_equal(np.asarray(u), np.asarray(v))


# ---- enhance --------------------------------------------------------------------------------------------------
F_E = N_B // 2 + 1


def _model(family):
    from drnmf_amd import layers
    if family == "lstm":
        torch.manual_seed(0)
        np.random.seed(0)
        return layers.build_lstm(dict(mask_value=-1., maxseq=200, input_dim=F_E, output_dim=F_E, K_layers=2,
                                      hidden_dim=48), device=DEV)
    r, K = 16, 3
    P = O.synth_problem(2, 4, F_E, r, seed=3)
    params = dict(input_dim=F_E, hidden_dim=2 * r, output_dim=F_E, mask_value=-1., maxseq=200, K_layers=K,
                  W=P["W"], alph=2 * r / 4.0, lam1=0.3, params_untied=["log_D", "log_alph"],
                  params_trainable=["log_D", "log_alph"])
    return layers.build_unfolded_snmf(params, device=DEV)


@pytest.mark.parametrize("family", ["lstm", "cell"])
def test_enhance_from_another_rate(ops, family):
    model = _model(family)
    wavs48 = [_signal(n, 60 + i, True) for i, n in enumerate((12000, 9001, 15100))]
    kw = dict(N=N_B, hop=HOP_B, dtype='float32', crop=True)
    got = model.enhance(wavs48, fs_in=48000, **kw)
    y, n_out = ops.resample(wavs48, 48000, 16000, device=DEV)
    want = model.enhance(y, lengths=n_out, **kw)
    assert [len(w) for w in got] == [R.out_len(len(w), 1, 3) for w in wavs48]
    for u, v in zip(got, want):
        assert u.dtype == np.float32 and np.array_equal(_bits(u), _bits(v))
    # a 2-D array with lengths, and the scores of a reference at fs
    pk = np.zeros((3, 15100), dtype=np.int16)
    for i, w in enumerate(wavs48):
        pk[i, :len(w)] = w
    ref = [(0.5 * w).astype(np.float32) for w in want]
    got2, S, labels = model.enhance(pk, lengths=[len(w) for w in wavs48], fs_in=48000, ref=ref, sdr_solver='device',
                                    **kw)
    want2, S2, _ = model.enhance(y, lengths=n_out, ref=ref, sdr_solver='device', **kw)
    for u, v in zip(got2, want):
        assert np.array_equal(_bits(u), _bits(v))
    assert np.array_equal(S, S2, equal_nan=True)
    # no rate, or the model's own: today's call
    wavs16 = [w[:3000] for w in wavs48]
    base = model.enhance(wavs16, **kw)
    for other in (model.enhance(wavs16, fs_in=None, **kw), model.enhance(wavs16, fs_in=16000, **kw),
                  model.enhance(wavs16, fs_in=8000, fs=8000, **kw)):
        for u, v in zip(base, other):
            assert np.array_equal(_bits(u), _bits(v))
    for bad in (0, 44101, 16000.5):
        with pytest.raises(ValueError):
            model.enhance(wavs16, fs_in=bad, **kw)
