"""The training-data front end on the MI355X (include/drnmf_dataset.h): ops.wavs_to_tensors / wavs_to_frames
bitwise against the path composed of ops.stft per signal and data.reshape_and_pad_stacks, the clamps of the raw
entry points, a table of more than 65 535 sequences, and fit_wavs against fit on the same tensors."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [(512, 128, 7), (1024, 256, 7), (256, 64, 5)]


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _frames(n, N, hop):
    return -(-n // hop) + N // hop + 1


def _clean_lengths(N, hop, maxlen):
    """Clean lengths whose frame counts ceil(len / hop) + N / hop + 1 hit: below maxlen (a signal shorter than one
    window), exactly maxlen, maxlen + 1, exactly 2 maxlen, and 4 maxlen + 1 (five pieces).  For (512, 128, 7): 1,
    256, 300, 1150, 3001 samples = 6, 7, 8, 14, 29 frames.  One sample already has N / hop + 2 frames; where that
    is above maxlen (N = 256, hop = 64, maxlen = 5) the first two branches do not exist and the one-sample signal
    is the maxlen + 1 case."""
    base = N // hop + 1
    lens = [1]
    for nf, back in ((maxlen, 0), (maxlen + 1, hop - hop // 3 - 2), (2 * maxlen, 2), (4 * maxlen + 1, hop // 2 + 7)):
        if nf - base >= 1:
            lens.append((nf - base) * hop - back)
            assert _frames(lens[-1], N, hop) == nf
    assert lens[0] < N and _frames(1, N, hop) == base + 1 <= maxlen + 1
    if (N, hop, maxlen) == (512, 128, 7):
        assert lens == [1, 256, 300, 1150, 3001]
    return lens


def _pairs(N, hop, maxlen, int16):
    """Every clean length with a noisy partner of the same length, one 300 samples (more than two hops) longer,
    and one 50 samples shorter where that keeps the frame count."""
    rng = np.random.default_rng(N + hop + int(int16))
    noisy, clean = [], []
    for n in _clean_lengths(N, hop, maxlen):
        for m in (n, n + 300, n - 50):
            if m < 1 or _frames(m, N, hop) < _frames(n, N, hop):
                continue
            for arr, k in ((clean, n), (noisy, m)):
                if int16:
                    arr.append(rng.integers(-20000, 20000, size=k).astype(np.int16))
                else:
                    arr.append((0.3 * rng.standard_normal(k)).astype(np.float32))
    assert len(clean) >= 9
    assert any(len(x) < len(y) for x, y in zip(noisy, clean))
    assert max(len(v) for v in noisy) % 2 == 1 or max(len(v) for v in clean) % 2 == 1      # an odd stride
    return noisy, clean


_composed_cache = {}


def _composed(ops, N, hop, maxlen, int16):
    """The path a caller had to write before: ops.stft per signal to the host, the noisy stack cut to the clean
    one's frame count, data.reshape_and_pad_stacks with pad -1.  Computed once per case and never modified."""
    key = (N, hop, maxlen, int16)
    if key not in _composed_cache:
        from drnmf_amd import data
        noisy, clean = _pairs(N, hop, maxlen, int16)
        xs, ys, fidx, t = [], [], [], 0
        for xw, yw in zip(noisy, clean):
            my = ops.stft(torch.from_numpy(yw).to(DEV), N=N, hop=hop, want_mag=True)[2][0].cpu().numpy()
            mx = ops.stft(torch.from_numpy(xw).to(DEV), N=N, hop=hop, want_mag=True)[2][0].cpu().numpy()
            assert mx.shape[0] >= my.shape[0] == _frames(len(yw), N, hop)
            xs.append(mx[:my.shape[0]].T)
            ys.append(my.T)
            fidx.append((t, t + my.shape[0]))
            t += my.shape[0]
        xs, ys, fidx = np.concatenate(xs, axis=1), np.concatenate(ys, axis=1), np.asarray(fidx)
        x, y, mask = data.reshape_and_pad_stacks(xs, ys, fidx, pad_value=-1.0, maxlen=maxlen)
        assert x.dtype == np.float32
        for a in (x, y, mask, xs, ys):
            a.setflags(write=False)
        _composed_cache[key] = (noisy, clean, x, y, mask, xs, ys)
    return _composed_cache[key]


def _same_bits(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32),
                                                                                      b.view(np.uint32))


@pytest.mark.parametrize("int16", [True, False], ids=["int16", "float32"])
@pytest.mark.parametrize("N,hop,maxlen", CASES)
def test_mag_tensors_are_bitwise_the_composed_path(ops, N, hop, maxlen, int16):
    noisy, clean, x0, y0, m0, _, _ = _composed(ops, N, hop, maxlen, int16)
    x, y, w = ops.wavs_to_tensors(noisy, clean, N=N, hop=hop, maxlen=maxlen, device=DEV)
    assert x.is_cuda and tuple(w.shape) == x.shape[:2] and x.shape[1] == maxlen
    assert x.shape[0] == sum(-(-_frames(len(c), N, hop) // maxlen) for c in clean)     # no empty trailing piece
    assert _same_bits(x, x0) and _same_bits(y, y0) and _same_bits(w, m0[:, :, 0])


@pytest.mark.parametrize("N,hop,maxlen", CASES)
def test_mag_tensors_without_chunking(ops, N, hop, maxlen):
    from drnmf_amd import data
    noisy, clean, _, _, _, xs, ys = _composed(ops, N, hop, maxlen, True)
    nf = np.array([_frames(len(c), N, hop) for c in clean])
    ends = np.cumsum(nf)
    fidx = np.stack([ends - nf, ends], axis=1)
    for ml in (None, int(nf.max()) + 3):
        x0, y0, m0 = data.reshape_and_pad_stacks(xs, ys, fidx, pad_value=-1.0, maxlen=ml)
        x, y, w = ops.wavs_to_tensors(noisy, clean, N=N, hop=hop, maxlen=ml, device=DEV)
        assert x.shape == (len(clean), int(nf.max()), N // 2 + 1)
        assert _same_bits(x, x0) and _same_bits(y, y0) and _same_bits(w, m0[:, :, 0])


def _ulps(got, want):
    """|got - want| in units of the float32 spacing at want."""
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


@pytest.mark.parametrize("N,hop,maxlen", CASES)
def test_logmag_tensors(ops, N, hop, maxlen):
    """Padding and weights bitwise; valid bins against numpy's float32 log(1 + m) of the device's own 'mag'
    output, within 4 float32 ulps of the result: both logf's are specified to about 1 ulp and the rounding of
    1 + m is common to both sides; the bound is twice their sum."""
    noisy, clean, x0, y0, m0, _, _ = _composed(ops, N, hop, maxlen, True)
    x, y, w = ops.wavs_to_tensors(noisy, clean, N=N, hop=hop, maxlen=maxlen, transform="logmag", device=DEV)
    assert _same_bits(w, m0[:, :, 0])
    valid = m0[:, :, 0] == 1.0
    worst = 0.0
    for got, mag in ((x.cpu().numpy(), x0), (y.cpu().numpy(), y0)):
        assert np.all(got[~valid] == np.float32(-1.0))
        want = np.log(np.float32(1) + mag[valid])
        assert want.dtype == np.float32
        g = got[valid]
        nz = want != 0
        assert np.array_equal(g[~nz], want[~nz])                    # log(1 + 0) = 0 exactly
        worst = max(worst, float(_ulps(g[nz], want[nz]).max()))
    print("logmag: max error %.2f ulp" % worst)
    assert worst <= 4.0, worst


@pytest.mark.parametrize("N,hop,maxlen", CASES)
def test_packed_frames_are_the_masked_frames_of_the_tensors(ops, N, hop, maxlen):
    from drnmf_amd import data
    noisy, clean, x0, y0, m0, xs, ys = _composed(ops, N, hop, maxlen, True)
    xf, yf = ops.wavs_to_frames(noisy, clean, N, hop)
    assert _same_bits(xf, np.ascontiguousarray(data.masked_seqs_to_frames(x0, m0).T))
    assert _same_bits(yf, np.ascontiguousarray(data.masked_seqs_to_frames(y0, m0).T))
    assert xf.shape[0] == xs.shape[1]
    xl, yl = ops.wavs_to_frames(noisy, clean, N, hop, transform="logmag")
    x, y, w = ops.wavs_to_tensors(noisy, clean, N=N, hop=hop, maxlen=maxlen, transform="logmag", device=DEV)
    keep = w.reshape(-1) == 1
    assert torch.equal(xl, x.reshape(-1, x.shape[2])[keep]) and torch.equal(yl, y.reshape(-1, y.shape[2])[keep])


@pytest.mark.parametrize("N,hop,maxlen", CASES)
def test_an_utterance_is_bitwise_independent_of_its_table(ops, N, hop, maxlen):
    noisy, clean, x0, y0, m0, _, _ = _composed(ops, N, hop, maxlen, False)
    u = max(i for i in range(len(clean)) if len(noisy[i]) == len(clean[i]) + 300)     # the five-piece one
    nf = _frames(len(clean[u]), N, hop)
    first = sum(-(-_frames(len(c), N, hop) // maxlen) for c in clean[:u])
    pieces = -(-nf // maxlen)
    # alone
    x, y, w = ops.wavs_to_tensors([noisy[u]], [clean[u]], N=N, hop=hop, maxlen=maxlen, device=DEV)
    assert _same_bits(x, x0[first:first + pieces]) and _same_bits(y, y0[first:first + pieces])
    # at another table position and another T
    order = [u] + [i for i in range(len(clean)) if i != u]
    T2 = maxlen + 2
    x, y, w = ops.wavs_to_tensors([noisy[i] for i in order], [clean[i] for i in order], N=N, hop=hop, maxlen=T2,
                                  device=DEV)
    p2 = -(-nf // T2)
    flat = lambda a, p, T: (a[:p].cpu().numpy() if isinstance(a, torch.Tensor) else a[first:first + p]) \
        .reshape(p * T, -1)[:nf]
    assert np.array_equal(w[:p2].cpu().numpy().reshape(-1)[:nf], np.ones(nf, np.float32))
    assert _same_bits(flat(x, p2, T2), flat(x0, pieces, maxlen))
    assert _same_bits(flat(y, p2, T2), flat(y0, pieces, maxlen))
    # and on a second run
    xb, yb, wb = ops.wavs_to_tensors([noisy[i] for i in order], [clean[i] for i in order], N=N, hop=hop, maxlen=T2,
                                     device=DEV)
    assert torch.equal(x, xb) and torch.equal(y, yb) and torch.equal(w, wb)


def _canaried(shape, extra=4096):
    """A float32 buffer of prod(shape) elements with `extra` canary elements on either side."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * extra,), 12345.0, dtype=torch.float32, device=DEV)
    return whole, whole[extra:extra + n].view(*shape), extra


def _canaries_intact(whole, extra):
    return bool((whole[:extra] == 12345.0).all()) and bool((whole[-extra:] == 12345.0).all())


@pytest.mark.parametrize("N,hop", [(512, 128), (256, 64)])
def test_clamps_of_the_raw_entry_points(ops, N, hop):
    F, T = N // 2 + 1, 9
    rng = np.random.default_rng(N)
    n_sig, sx, sy = 3, 2001, 1801
    px = torch.from_numpy(rng.integers(-20000, 20000, size=(n_sig, sx)).astype(np.int16)).to(DEV)
    py = torch.from_numpy(rng.integers(-20000, 20000, size=(n_sig, sy)).astype(np.int16)).to(DEV)
    # signal 1: lengths far above the strides behave as the strides
    lx = torch.tensor([1500, 10 ** 12, 900], dtype=torch.int64, device=DEV)
    ly = torch.tensor([1200, 10 ** 12, 900], dtype=torch.int64, device=DEV)
    rows = [(0, 0), (-1, 0), (n_sig, 0), (2, -1), (1, 0), (1, T), (0, 10 ** 6), (-2 ** 31, 2 ** 31 - 1)]
    table = torch.tensor(rows, dtype=torch.int32, device=DEV)
    bufs = [_canaried((len(rows), T, F)), _canaried((len(rows), T, F)), _canaried((len(rows), T))]
    (xw, x, e), (yw, y, _), (ww, w, _) = bufs
    ops.stft_pair_chunks_enqueue(px, py, lx, ly, table, T, N, hop, "mag", -1.0, x, y, w)
    torch.cuda.synchronize()
    assert all(_canaries_intact(b[0], b[2]) for b in bufs)
    for k in (1, 2, 3, 6, 7):                                       # all padding, zero weights
        assert bool((x[k] == -1).all()) and bool((y[k] == -1).all()) and bool((w[k] == 0).all()), k
    magx = ops.stft(px[1], N=N, hop=hop, want_mag=True)[2][0]       # the whole row = length `stride`
    magy = ops.stft(py[1], N=N, hop=hop, want_mag=True)[2][0]
    nf = _frames(sy, N, hop)
    assert nf > 2 * T - 4
    got_x, got_y = torch.cat([x[4], x[5]])[:nf], torch.cat([y[4], y[5]])[:nf]
    assert torch.equal(got_x[:min(nf, 2 * T)], magx[:min(nf, 2 * T)])
    assert torch.equal(got_y[:min(nf, 2 * T)], magy[:min(nf, 2 * T)])
    assert bool((w[4] == 1).all()) and torch.equal(w[5], (torch.arange(T, device=DEV) + T < nf).float())
    assert torch.equal(y[0][:min(T, _frames(1200, N, hop))],
                       ops.stft(py[0, :1200], N=N, hop=hop, want_mag=True)[2][0][:T])

    # packed mode: the same clamps; a row0 that leaves too few rows drops frames instead of writing past the end
    nfs = [_frames(1200, N, hop), nf, _frames(900, N, hop)]
    total = sum(nfs)
    row0 = torch.tensor([0, nfs[0], nfs[0] + nfs[1]], dtype=torch.int64, device=DEV)
    (xw, xf, e), (yw, yf, _) = _canaried((total, F)), _canaried((total, F))
    ops.stft_pair_frames_enqueue(px, py, lx, ly, row0, N, hop, "mag", xf, yf)
    torch.cuda.synchronize()
    assert _canaries_intact(xw, e) and _canaries_intact(yw, e)
    assert torch.equal(xf[nfs[0]:nfs[0] + nf], magx[:nf]) and torch.equal(yf[nfs[0]:nfs[0] + nf], magy)
    assert torch.equal(yf[:nfs[0]], ops.stft(py[0, :1200], N=N, hop=hop, want_mag=True)[2][0])
    short = total - 5
    bad = torch.tensor([0, -3, short - 2], dtype=torch.int64, device=DEV)
    (xw, xf, e), (yw, yf, _) = _canaried((short, F)), _canaried((short, F))
    ops.stft_pair_frames_enqueue(px, py, lx, ly, bad, N, hop, "mag", xf, yf)
    torch.cuda.synchronize()
    assert _canaries_intact(xw, e) and _canaries_intact(yw, e)
    assert bool((xf[nfs[0]:short - 2] == 12345.0).all())            # signal 1 (row0 < 0) wrote nothing


def test_more_than_65535_sequences(ops):
    """One pair of 70 000 * 16 samples at N = 64, hop = 16, maxlen = 1: 70 005 sequences of one frame."""
    N, hop, n = 64, 16, 70000 * 16
    rng = np.random.default_rng(6)
    clean = (0.3 * rng.standard_normal(n)).astype(np.float32)
    noisy = (clean + 0.1 * rng.standard_normal(n)).astype(np.float32)
    x, y, w = ops.wavs_to_tensors([noisy], [clean], N=N, hop=hop, maxlen=1, device=DEV)
    assert tuple(x.shape) == (70005, 1, 33) and tuple(w.shape) == (70005, 1)
    assert bool((w == 1).all())
    assert torch.equal(x[:, 0], ops.stft(torch.from_numpy(noisy).to(DEV), N=N, hop=hop, want_mag=True)[2][0])
    assert torch.equal(y[:, 0], ops.stft(torch.from_numpy(clean).to(DEV), N=N, hop=hop, want_mag=True)[2][0])


def test_bad_pairs_raise_and_enqueue_nothing(ops):
    a, b = np.zeros(1000, np.int16), np.zeros(700, np.int16)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    for fn in (lambda p, q: ops.wavs_to_tensors(p, q, device=DEV), lambda p, q: ops.wavs_to_frames(p, q, 512, 128)):
        with pytest.raises(ValueError):
            fn([a, a], [a])
        with pytest.raises(ValueError):
            fn([a, b], [a, a])                                      # 11 frames against 13
        with pytest.raises(ValueError):
            fn([], [])
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before      # not even a device buffer


F_E = 257


def _utterances(seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(int(0.3 * 16000), int(1.5 * 16000), size=12)
    noisy = [(rng.standard_normal(n) * 3000 * (1 + 0.5 * np.sin(np.arange(n) / 900.0))).astype(np.int16)
             for n in lens]
    clean = [(0.6 * w + 200 * rng.standard_normal(len(w))).astype(np.int16) for w in noisy]
    return noisy, clean


def _model(family, mask_value=-1.):
    from drnmf_amd import layers
    from oracle import drnmf_oracle as O
    torch.manual_seed(0)
    np.random.seed(0)
    if family == "snmf":
        r, K = 16, 3
        P = O.synth_problem(2, 4, F_E, r, seed=3)
        params = dict(input_dim=F_E, hidden_dim=2 * r, output_dim=F_E, mask_value=mask_value, maxseq=200,
                      K_layers=K, W=P["W"], alph=2 * r / 4.0, lam1=0.3, params_untied=["log_D", "log_alph"],
                      params_trainable=["log_D", "log_alph"])
        m = layers.build_unfolded_snmf(params, device=DEV)
    else:
        m = layers.build_lstm(dict(mask_value=mask_value, maxseq=200, input_dim=F_E, output_dim=F_E, K_layers=2,
                                   hidden_dim=48), device=DEV)
    m.compile(lr=1e-3)
    return m


@pytest.mark.parametrize("family", ["snmf", "lstm"])
def test_fit_wavs_is_fit_on_the_tensors(ops, family):
    noisy, clean = _utterances(4)
    noisy_v, clean_v = (v[:4] for v in _utterances(9))
    kw = dict(batch_size=5, epochs=2, seed=123)
    x, y, w = ops.wavs_to_tensors(noisy, clean, maxlen=40, device=DEV)
    val = ops.wavs_to_tensors(noisy_v, clean_v, maxlen=40, device=DEV)
    assert x.shape[1] == 40 and x.shape[0] > 12
    runs = [_model(family).fit(x, y, sample_weight=w, validation_data=val, **kw) for _ in range(2)]
    got = _model(family).fit_wavs(noisy, clean, maxlen=40, validation_wavs=(noisy_v, clean_v), **kw)
    for key in ("loss", "val_loss"):
        a, b, g = (np.array([float(v) for v in h[key]]) for h in (runs[0], runs[1], got))
        assert a.shape == (2,) and np.all(np.isfinite(a)) and np.all(a > 0)
        d = np.abs(a - b)                                          # what two runs of fit on identical tensors differ by
        print(family, key, "repeat-run difference", d, "fit_wavs - fit", g - a)
        assert np.all(np.abs(g - a) <= d), (key, g, a, d)          # d == 0: exact equality
    with pytest.raises(ValueError, match="masks"):
        _model(family, mask_value=0.).fit_wavs(noisy, clean, maxlen=40, **kw)
