"""The training targets on the MI355X (include/drnmf_target.h): ops.wavs_to_tensors(..., target='psa' / 'tpsa')
against the device's own spectra (tight: the four roundings of the definition), against the fp64 spectra of the
waveforms (independent: sign, member order, every bin), bitwise independence of the table, x and w bitwise those
of target='mag', and fit_wavs(..., target=) against fit on the same tensors.  Sizes and pairs: tests/psa_ref.py."""
import functools

import numpy as np
import pytest
import torch

import psa_ref as P
import stft_hops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TYPES = dict(argnames="int16", argvalues=[True, False], ids=["int16", "float32"])
SIZES = dict(argnames="N,hop", argvalues=R.PAIR_SIZES, ids=R.ids(R.PAIR_SIZES))


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _tensors(N, hop, int16, target):
    """(x, y, w) of the size's pairs as host arrays, once per target; never modified."""
    from drnmf_amd import ops
    _, noisy, clean, _, _ = P.pairs(N, hop, int16)
    out = ops.wavs_to_tensors(list(noisy), list(clean), N=N, hop=hop, maxlen=P.MAXLEN, device=DEV, target=target)
    return tuple(R._frozen(t.cpu().numpy()) for t in out)


@functools.lru_cache(maxsize=None)
def _device_spectra(N, hop, int16):
    """Per pair (re_x, im_x, m_x, re_s, im_s) as ops.stft writes them, float32 [nf, F] with nf the clean member's
    frame count; never modified."""
    from drnmf_amd import ops
    _, noisy, clean, _, _ = P.pairs(N, hop, int16)
    out = []
    for xw, sw in zip(noisy, clean):
        nf = R.frames(len(sw), N, hop)
        rx, ix, mx = (t[0, :nf].cpu().numpy() for t in
                      ops.stft(torch.from_numpy(np.ascontiguousarray(xw)).to(DEV), N=N, hop=hop, want_mag=True))
        rs, i_s = (t[0].cpu().numpy() for t in ops.stft(torch.from_numpy(np.ascontiguousarray(sw)).to(DEV), N=N,
                                                         hop=hop))
        assert rs.shape == rx.shape == (nf, N // 2 + 1)
        out.append(tuple(R._frozen(a) for a in (rx, ix, mx, rs, i_s)))
    return tuple(out)


def _per_pair(a, w, clean, N, hop):
    """The valid frames of a tensor [n_seq, T, F], utterance after utterance: a list of [nf, F]."""
    flat = a.reshape(-1, a.shape[2])[w.reshape(-1) == 1]
    nfs = [R.frames(len(c), N, hop) for c in clean]
    assert flat.shape[0] == sum(nfs)
    return np.split(flat, np.cumsum(nfs)[:-1])


def _same_bits(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32),
                                                                                      b.view(np.uint32))


@pytest.mark.parametrize(**TYPES)
@pytest.mark.parametrize(**SIZES)
def test_x_and_w_do_not_depend_on_the_target(ops, N, hop, int16):
    _, noisy, clean, _, _ = P.pairs(N, hop, int16)
    x0, y0, w0 = _tensors(N, hop, int16, "mag")
    assert x0.shape[1] == P.MAXLEN and x0.shape[0] == sum(-(-R.frames(len(c), N, hop) // P.MAXLEN) for c in clean)
    assert np.any(w0 == 0) and np.all(w0[:, 0] == 1)                  # sequences are cut, the last ones padded
    mx = [s[2] for s in _device_spectra(N, hop, int16)]
    assert all(_same_bits(a, b) for a, b in zip(_per_pair(x0, w0, clean, N, hop), mx))     # x is drnmf_stft's magnitude
    for target in P.TARGETS:
        x, y, w = _tensors(N, hop, int16, target)
        assert _same_bits(x, x0) and _same_bits(w, w0), target
        assert np.all(y[w == 0] == np.float32(-1.0)) and np.all(x[w == 0] == np.float32(-1.0))
    # target = 'mag' through the new entry point is the existing entry point, bit for bit
    pcm_x, len_x = ops._upload_wav_side([np.asarray(v) for v in noisy], noisy[0].dtype, torch.device(DEV))
    pcm_y, len_y = ops._upload_wav_side([np.asarray(v) for v in clean], clean[0].dtype, torch.device(DEV))
    from drnmf_amd import data
    table, T = data.sequence_table_from_lengths(np.array([R.frames(len(c), N, hop) for c in clean]), P.MAXLEN)
    table_d = torch.from_numpy(table).to(DEV)
    x, y, w = (torch.full(s, 7.0, dtype=torch.float32, device=DEV) for s in (x0.shape, x0.shape, w0.shape))
    ops.stft_pair_target_enqueue(pcm_x, pcm_y, len_x, len_y, table_d, T, N, hop, "mag", "mag", -1.0, x, y, w)
    assert _same_bits(x, x0) and _same_bits(y, y0) and _same_bits(w, w0)


@pytest.mark.parametrize(**TYPES)
@pytest.mark.parametrize(**SIZES)
def test_targets_against_the_device_spectra(ops, N, hop, int16):
    """|y - p64| <= 2^-21 |S| + 1e-37 on EVERY valid bin, p64 the fp64 value of the definition on the device's own
    float32 re, im and m_x.  Two products, one sum and one division round once each and |re_s re_x| + |im_s im_x|
    <= |S| m_x, so the error is at most 4 * 2^-24 |S| = 2^-22 |S|; the bound leaves a factor 2 for another
    association of the same four operations."""
    kinds, noisy, clean, _, _ = P.pairs(N, hop, int16)
    spectra = _device_spectra(N, hop, int16)
    silent = 0
    for target in P.TARGETS:
        x, y, w = _tensors(N, hop, int16, target)
        assert np.all(np.isfinite(y))
        for kind, got, xm, (rx, ix, mx, rs, i_s) in zip(kinds, _per_pair(y, w, clean, N, hop),
                                                        _per_pair(x, w, clean, N, hop), spectra):
            S, X = rs.astype(np.float64) + 1j * i_s.astype(np.float64), rx.astype(np.float64) + 1j * ix.astype(np.float64)
            want = P.target(target, S, X, mx)
            err, bound = np.abs(got.astype(np.float64) - want), 2.0 ** -21 * np.abs(S) + 1e-37
            print("N=%d hop=%d %s %s %-7s max err / |S| = %.3g (bound %.3g)"
                  % (N, hop, "int16" if int16 else "float32", target, kind,
                     float(np.max(err / np.maximum(np.abs(S), 1e-30))), 2.0 ** -21))
            assert np.all(err <= bound), (target, kind, float(np.max(err - bound)))
            assert np.all(got[mx == 0] == 0)                          # m_x == 0: exactly 0
            if target == "tpsa":
                assert np.all(got >= 0) and np.all(got <= xm)         # exactly, on every valid bin
            if kind in ("zeros", "early"):
                silent += int(np.sum((mx == 0).all(axis=1) & (np.abs(S) > 0).any(axis=1)))
            if kind == "negated" and target == "tpsa":
                assert np.all(got == 0)
    assert silent > 0                  # whole frames in which the noisy member is silent under a live clean one


@pytest.mark.parametrize(**TYPES)
@pytest.mark.parametrize(**SIZES)
def test_psa_against_fp64_from_the_waveforms(ops, N, hop, int16):
    """max |y_psa x - Re(S64 conj X64)| <= 4 TOL_FWD max|S64| max|X64| per pair: y x = re_s re_x + im_s im_x is the
    well-conditioned product, each factor carries TOL_FWD, and the 4 is a factor 2 over their sum.  A wrong sign, a
    swapped member or a dropped bin 0 / N/2 fails here."""
    kinds, noisy, clean, X64, S64 = P.pairs(N, hop, int16)
    x, y, w = _tensors(N, hop, int16, "psa")
    for kind, got, xm, X, S in zip(kinds, _per_pair(y, w, clean, N, hop), _per_pair(x, w, clean, N, hop), X64, S64):
        want = (S * np.conj(X)).real.T
        err = float(np.max(np.abs(got.astype(np.float64) * xm.astype(np.float64) - want)))
        bound = 4 * R.TOL_FWD * float(np.max(np.abs(S))) * float(np.max(np.abs(X)))
        print("N=%d hop=%d %s %-7s max |y x - Re(S conj X)| = %.3g (bound %.3g)"
              % (N, hop, "int16" if int16 else "float32", kind, err, bound))
        assert err <= bound, (kind, err, bound)


@pytest.mark.parametrize("target", P.TARGETS)
@pytest.mark.parametrize(**SIZES)
def test_a_pair_is_bitwise_independent_of_its_table(ops, N, hop, target):
    kinds, noisy, clean, _, _ = P.pairs(N, hop, False)
    _, y0, w0 = _tensors(N, hop, False, target)
    u = kinds.index("zeros")                                          # the longest one
    nf = R.frames(len(clean[u]), N, hop)
    want = _per_pair(y0, w0, clean, N, hop)[u]
    # alone
    x, y, w = ops.wavs_to_tensors([noisy[u]], [clean[u]], N=N, hop=hop, maxlen=P.MAXLEN, device=DEV, target=target)
    assert _same_bits(_per_pair(y.cpu().numpy(), w.cpu().numpy(), [clean[u]], N, hop)[0], want)
    # at another table position and another T
    order = [u] + [i for i in range(len(clean)) if i != u]
    T2 = P.MAXLEN + 2
    x, y, w = ops.wavs_to_tensors([noisy[i] for i in order], [clean[i] for i in order], N=N, hop=hop, maxlen=T2,
                                  device=DEV, target=target)
    assert y.shape[1] == T2
    got = _per_pair(y.cpu().numpy(), w.cpu().numpy(), [clean[i] for i in order], N, hop)[0]
    assert got.shape == (nf, N // 2 + 1) and _same_bits(got, want)


# ---- fit_wavs ------------------------------------------------------------------------------------------------------
from test_gpu_dataset import _model, _utterances              # noqa: E402  (helpers only; they import cleanly)


def _weights(model):
    return [np.asarray(v) for v in model.get_weights()]


@pytest.mark.parametrize("family", ["snmf", "lstm"])
def test_fit_wavs_with_a_target_is_fit_on_the_tensors(ops, family):
    """As test_gpu_dataset.test_fit_wavs_is_fit_on_the_tensors, with target='tpsa' on the training AND the validation
    side: history and weights are those of fit on the 'tpsa' tensors (within what two runs of fit on identical
    tensors differ by), and val_loss is not the 'mag' run's."""
    noisy, clean = _utterances(4)
    noisy_v, clean_v = (v[:4] for v in _utterances(9))
    kw = dict(batch_size=5, epochs=2, seed=123)
    x, y, w = ops.wavs_to_tensors(noisy, clean, maxlen=40, device=DEV, target="tpsa")
    val = ops.wavs_to_tensors(noisy_v, clean_v, maxlen=40, device=DEV, target="tpsa")
    models = [_model(family) for _ in range(2)]
    runs = [m.fit(x, y, sample_weight=w, validation_data=val, **kw) for m in models]
    mine = _model(family)
    got = mine.fit_wavs(noisy, clean, maxlen=40, validation_wavs=(noisy_v, clean_v), target="tpsa", **kw)
    for key in ("loss", "val_loss"):
        a, b, g = (np.array([float(v) for v in h[key]]) for h in (runs[0], runs[1], got))
        assert a.shape == (2,) and np.all(np.isfinite(a)) and np.all(a > 0)
        d = np.abs(a - b)                                          # what two runs of fit on identical tensors differ by
        print(family, key, "repeat-run difference", d, "fit_wavs - fit", g - a)
        assert np.all(np.abs(g - a) <= d), (key, g, a, d)          # d == 0: exact equality
    for wa, wb, wg in zip(_weights(models[0]), _weights(models[1]), _weights(mine)):
        assert np.all(np.abs(wg - wa) <= np.abs(wa - wb))
    ref = _model(family).fit_wavs(noisy, clean, maxlen=40, validation_wavs=(noisy_v, clean_v), **kw)
    assert all(float(g) != float(r) for g, r in zip(got["val_loss"], ref["val_loss"]))    # the validation side took it
    with pytest.raises(ValueError, match="transform 'mag' only"):
        _model(family).fit_wavs(noisy, clean, maxlen=40, transform="logmag", target="psa", **kw)
