"""The STFT and inverse kernels of csrc/stft.hip and csrc/stft_stream.h on the MI355X at hops other than N/4: the
grid of tests/stft_hops_ref.py (the default hop N/2, hop = N, hop > N, hops that do not divide N or 2048, an odd hop,
N/64, and the general-path sizes 128 / 2048 / 4096) through the ragged, batched, paired-dataset and streaming entry
points, against the oracle's stft_mc / reconstruct at the project's own bounds (2e-5 max|S| forward, 1e-4 max|ref|
inverse) and bitwise where the headers promise it.  Every test prints the largest relative error it measured.

Which test a wrong kernel fails (reasoned from the code):
  fft_lds without its odd-log2 first stage   the forward tests at N = 128 / 2048 and every inverse test at
                                             (512, 600), (128, *), (2048, 512)
  the wmax guard of the fused inverse dropped test_inverse_with_T_below_a_rows_frames at (512, 160): only a T that
                                             cuts a row makes f_hi stop inside a group of four, where the waves past
                                             wmax still hold the frames of the group before
  the aligned 8-byte load taken regardless   the ragged and batched forward tests at (512, 129) (and 1025) run it:
  of the first sample's parity               every other interior frame then starts at an odd element.  They fail
                                             where such a load faults or drops the low address bits; a device that
                                             serves misaligned global loads returns the same values, and then
                                             nothing can tell the two paths apart -- what the grid adds is that
                                             BOTH paths of one signal are compared with the oracle
A run of 2048 samples at every hop, or f_lo = s0 / hop without the + 1, changes no value as long as the host and the
kernel agree on it (a sample's sum is over its own frames in ascending order whatever the run, and the extra frame
is rejected by the n < N test); what (512, 160) and (1024, 1000) pin is that run < 2048 with its i < run guard, the
grid of ceil(stride / run) workgroups and the non-multiple output length give the oracle's samples."""
import functools

import numpy as np
import pytest
import torch

import stft_hops_ref as R
from oracle import drnmf_oracle as O
from test_stream_host import cut_schedule

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TYPES = dict(argnames="int16", argvalues=[True, False], ids=["int16", "float32"])


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _ops():
    from drnmf_amd import ops
    return ops


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)     # (a copy: the shared references are read-only)


def _sizes(sizes):
    return dict(argnames="N,hop", argvalues=sizes, ids=R.ids(sizes))


@functools.lru_cache(maxsize=None)
def _device_forward(N, hop, int16):
    """ops.stft_ragged of the whole batch of a size in its own order, once: (x, re, im, nf)."""
    lens, pcm = R.signals(N, hop, int16)
    return _ops().stft_ragged(_t(pcm), lens, N=N, hop=hop)


def _forward_errors(re, im, x, S):
    """Relative errors of one row's device frames [nf, F] against the oracle spectrum S [F, nf]."""
    scale = float(np.max(np.abs(S)))
    mag = np.sqrt(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2)
    errs = [float(np.max(np.abs(re.T - S.real))), float(np.max(np.abs(im.T - S.imag))),
            float(np.max(np.abs(x - mag)))]
    if scale == 0.0:                                          # a lone sample under the window's zero: exact zeros
        return [0.0 if e == 0.0 else float("inf") for e in errs]
    return [e / scale for e in errs]


# ---- ragged forward --------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**TYPES)
@pytest.mark.parametrize(**_sizes(R.SIZES))
def test_ragged_forward_matches_stft_mc_per_row(ops, N, hop, int16):
    lens, pcm = R.signals(N, hop, int16)
    n = len(lens)
    idx = [n - 2, 0, n - 1, 3, 2]                             # shuffled, part of the batch
    T = max(R.frames(lens[i], N, hop) for i in idx) + 5
    x, re, im, nf = ops.stft_ragged(_t(pcm), lens, sig_index=idx, T=T, N=N, hop=hop, mask_value=-1.0)
    x, re, im = x.cpu().numpy(), re.cpu().numpy(), im.cpu().numpy()
    assert x.shape == (len(idx), T, N // 2 + 1)
    S = R.spectra(N, hop, int16)
    worst = 0.0
    for k, i in enumerate(idx):
        f = int(nf[k])
        assert f == S[i].shape[1]
        errs = _forward_errors(re[k, :f], im[k, :f], x[k, :f], S[i])
        worst = max(worst, max(errs))
        assert max(errs) <= R.TOL_FWD, (i, lens[i], errs)
        assert np.all(x[k, f:] == np.float32(-1.0))
    print("ragged forward N=%d hop=%d %s: max error %.3e of max|S|" % (N, hop, "int16" if int16 else "float32", worst))
    # the default gather list and T, another padding value
    x2, _, _, nf2 = ops.stft_ragged(_t(pcm), lens, N=N, hop=hop, mask_value=-7.5)
    assert x2.shape[:2] == (n, max(nf2))
    x2 = x2.cpu().numpy()
    for i in range(n):
        assert np.all(x2[i, int(nf2[i]):] == np.float32(-7.5))
        assert np.all(x2[i, :int(nf2[i])] >= 0)


# ---- ragged inverse --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crop", [False, True], ids=["full", "crop"])
@pytest.mark.parametrize(**_sizes(R.SIZES))
def test_ragged_inverse_matches_reconstruct_per_row(ops, N, hop, crop):
    lens, pcm = R.signals(N, hop, False)
    n, F = len(lens), N // 2 + 1
    idx = [n - 1, 1, 4, 0] + ([n - 2] if n - 2 != 4 else []) + [2]       # shuffled; row 3 is not named
    _, re_all, im_all, nf_all = _device_forward(N, hop, False)
    sel = torch.tensor(idx, device=DEV)
    re, im = re_all[sel].contiguous(), im_all[sel].contiguous()
    T = re.shape[1]
    mask = np.random.default_rng(N + hop).random((len(idx), T, F)).astype(np.float32)      # junk behind a row's frames
    for k, i in enumerate(idx):
        mask[k, :int(nf_all[i])] = R.masks(N, hop)[i]
    n_out = ops.ragged_out_lengths(lens, N, hop, crop)
    width = int(max(R.out_length(m, N, hop) for m in lens)) + 2 * hop + 3
    out = torch.full((n, width), 7.0, dtype=torch.float32, device=DEV)
    y = ops.istft_ragged(re, im, _t(mask), lens, N, hop, sig_index=idx, out=out, crop=crop).cpu().numpy()
    refs = R.reconstructions(N, hop, True)
    worst = 0.0
    for i in idx:
        ref = refs[i][:lens[i]] if crop else refs[i]
        assert ref.shape[0] == n_out[i] == R.out_length(lens[i], N, hop, crop)
        if N % hop and hop < N and not crop:
            assert n_out[i] != -(-lens[i] // hop) * hop       # not the rule of the hops that divide N
        err = R.rel_err(y[i, :n_out[i]], ref)
        worst = max(worst, err)
        assert err <= R.TOL_INV, (i, lens[i], err)
        assert np.all(y[i, n_out[i]:] == 0.0)
        if hop > N:                                           # samples under no frame
            assert np.all(y[i, :n_out[i]][R.uncovered(n_out[i], N, hop)] == 0.0)
    assert np.all(y[3] == 7.0)                                # a row the gather list does not name is untouched
    print("ragged inverse N=%d hop=%d %s: max error %.3e of max|ref|" % (N, hop, "crop" if crop else "full", worst))
    # the allocating form
    y2 = ops.istft_ragged(re, im, _t(mask), lens, N, hop, sig_index=idx, crop=crop)
    assert y2.shape == (n, max(n_out))
    for i in idx:
        assert torch.equal(y2[i, :n_out[i]].cpu(), torch.from_numpy(y[i, :n_out[i]]))
    if not crop:                                              # once per size: no mask, the whole batch in order
        y0 = ops.istft_ragged(re_all, im_all, None, lens, N, hop).cpu().numpy()
        plain = R.reconstructions(N, hop, False)
        e0 = max(R.rel_err(y0[i, :n_out[i]], plain[i]) for i in range(n))
        print("ragged inverse N=%d hop=%d without a mask: max error %.3e of max|ref|" % (N, hop, e0))
        assert e0 <= R.TOL_INV, e0
        for i in range(n):
            assert np.all(y0[i, n_out[i]:] == 0.0)


@pytest.mark.parametrize("crop", [False, True], ids=["full", "crop"])
@pytest.mark.parametrize(**_sizes(R.T_CUT_SIZES))
def test_inverse_with_T_below_a_rows_frames(ops, N, hop, crop):
    """A slab whose T cuts the two long rows: the inverse must be O.reconstruct of the spectrum with the frames at or
    behind T zeroed (the nfe clamp of both inverse paths); the output lengths stay those of the rows' own lengths.
    T = 50 at (512, 160): the run of samples 5760 .. 7679 spans frames 37 .. 51, of which 37 .. 49 remain: thirteen,
    so the last group of four holds one live frame and three stale ones."""
    lens, _ = R.signals(N, hop, False)
    Tc = {(512, 160): 50, (128, 32): 200}[(N, hop)]
    nfs = [R.frames(m, N, hop) for m in lens]
    assert sum(f > Tc for f in nfs) == 2 and min(nfs) < Tc
    _, re, im, _ = _device_forward(N, hop, False)
    re, im = re[:, :Tc].contiguous(), im[:, :Tc].contiguous()
    mask = np.zeros((len(lens), Tc, N // 2 + 1), np.float32)
    for i, m in enumerate(R.masks(N, hop)):
        mask[i, :min(Tc, nfs[i])] = m[:Tc]
    y = ops.istft_ragged(re, im, _t(mask), lens, N, hop, crop=crop).cpu().numpy()
    n_out = ops.ragged_out_lengths(lens, N, hop, crop)
    S = R.spectra(N, hop, False)
    worst = 0.0
    for i, m in enumerate(lens):
        ref = R.reconstruct(S[i], R.masks(N, hop)[i], N, hop, nsampl=m if crop else None, keep_frames=Tc)
        assert ref.shape[0] == n_out[i]
        if nfs[i] > Tc:
            assert np.all(ref[Tc * hop:] == 0.0) and np.any(ref[:Tc * hop - N] != 0.0)
        err = R.rel_err(y[i, :n_out[i]], ref)
        worst = max(worst, err)
        assert err <= R.TOL_INV, (i, m, err)
        assert np.all(y[i, n_out[i]:] == 0.0)
    print("inverse with T=%d N=%d hop=%d %s: max error %.3e of max|ref|" % (Tc, N, hop, "crop" if crop else "full",
                                                                              worst))


# ---- batched entry points ----------------------------------------------------------------------------------------
@pytest.mark.parametrize(**TYPES)
@pytest.mark.parametrize(**_sizes(R.SIZES))
def test_batched_entry_points(ops, N, hop, int16):
    """ops.stft, ops.stft_mag and ops.istft_masked at equal lengths against the oracle, and the ragged forward of a
    row bitwise the batched one of that row alone (include/drnmf_dataset.h states it for the magnitude; re and im
    come out of the same frame body).  The inverses are each tied to the oracle only: ops.istft_masked is the
    two-stage path at every size while the ragged inverse of N = 512 / 1024 is the fused kernel, and no header
    promises that the two agree to the bit."""
    _, pcm = R.signals(N, hop, int16)
    w = O.sqrt_hann(N)
    F = N // 2 + 1
    for nsampl in R.equal_lengths(N, hop):
        rows = np.ascontiguousarray(pcm[:3, :nsampl])         # (the junk behind a short row's length is noise too)
        S = [O.stft_mc(R.as_float(r), N, hop, w) for r in rows]
        nf = S[0].shape[1]
        re, im, mag = ops.stft(_t(rows), N=N, hop=hop, want_mag=True)
        mag_only = ops.stft_mag(_t(rows), N=N, hop=hop)
        assert tuple(re.shape) == tuple(mag_only.shape) == (3, nf, F)
        ren, imn, magn, mon = (a.cpu().numpy() for a in (re, im, mag, mag_only))
        e_f = 0.0
        for r in range(3):
            e_f = max([e_f] + _forward_errors(ren[r], imn[r], magn[r], S[r]) +
                      _forward_errors(ren[r], imn[r], mon[r], S[r])[2:])
        assert e_f <= R.TOL_FWD, (nsampl, e_f)
        # ragged (odd stride, junk behind the length) against each row alone
        wide = np.concatenate([rows, pcm[:3, nsampl:nsampl + (2 if nsampl % 2 else 1)]], axis=1)
        assert wide.shape[1] % 2 == 1
        xr, rr, ir, nfr = ops.stft_ragged(_t(wide), [nsampl] * 3, N=N, hop=hop)
        assert list(nfr) == [nf] * 3
        for r in range(3):
            a_re, a_im, a_mag = ops.stft(_t(rows[r]), N=N, hop=hop, want_mag=True)
            assert torch.equal(rr[r], a_re[0]) and torch.equal(ir[r], a_im[0]) and torch.equal(xr[r], a_mag[0]), r
            assert torch.equal(a_re[0], re[r]) and torch.equal(a_im[0], im[r]) and torch.equal(a_mag[0], mag[r]), r
            assert torch.equal(ops.stft_mag(_t(rows[r]), N=N, hop=hop)[0], mag_only[r]), r
        e_i = 0.0
        if not int16:
            rng = np.random.default_rng(nsampl)
            mask = rng.random((3, nf, F)).astype(np.float32)
            n_out = R.out_length(nsampl, N, hop)
            y = ops.istft_masked(re, im, _t(mask), n_out, N, hop).cpu().numpy()
            y0 = ops.istft_masked(re, im, None, n_out, N, hop).cpu().numpy()
            assert y.shape == (3, n_out)
            for r in range(3):
                ref = R.reconstruct(S[r], mask[r], N, hop)
                assert ref.shape[0] == n_out
                e_i = max(e_i, R.rel_err(y[r], ref), R.rel_err(y0[r], R.reconstruct(S[r], None, N, hop)))
                if hop > N:
                    assert np.all(y[r][R.uncovered(n_out, N, hop)] == 0.0)
            assert e_i <= R.TOL_INV, (nsampl, e_i)
        print("batched N=%d hop=%d nsampl=%d %s: forward %.3e of max|S|, inverse %s of max|ref|"
              % (N, hop, nsampl, "int16" if int16 else "float32", e_f, "n/a" if int16 else "%.3e" % e_i))


# ---- batch independence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**TYPES)
@pytest.mark.parametrize(**_sizes(R.INDEPENDENCE_SIZES))
def test_a_row_is_bitwise_independent_of_its_batch(ops, N, hop, int16):
    lens, pcm = R.signals(N, hop, int16)
    nfs = [R.frames(m, N, hop) for m in lens]
    masks = R.masks(N, hop)

    def run(rows, T, order):
        """Signals `rows` as a batch of their own (other strides, positions and T); per signal (x, re, im, y, q)."""
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
            f = int(nf[k])
            res[rows[r]] = tuple(a.cpu().numpy() for a in (x[k, :f], re[k, :f], im[k, :f], y[r, :n_out[r]],
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
    print("independence N=%d hop=%d: %d rows bitwise alone, in the batch and in another slab (error 0)"
          % (N, hop, len(lens)))


# ---- paired dataset kernels ----------------------------------------------------------------------------------
from test_gpu_dataset import _composed, _same_bits, _ulps      # noqa: E402  (helpers only; they import cleanly)

MAXLEN = 7


@pytest.mark.parametrize(**TYPES)
@pytest.mark.parametrize(**_sizes(R.PAIR_SIZES))
def test_pair_tensors_are_bitwise_the_composed_path(ops, N, hop, int16):
    from drnmf_amd import data
    noisy, clean, x0, y0, m0, _, _ = _composed(ops, N, hop, MAXLEN, int16)
    x, y, w = ops.wavs_to_tensors(noisy, clean, N=N, hop=hop, maxlen=MAXLEN, device=DEV)
    assert x.shape[1] == MAXLEN
    assert x.shape[0] == sum(-(-R.frames(len(c), N, hop) // MAXLEN) for c in clean)
    assert _same_bits(x, x0) and _same_bits(y, y0) and _same_bits(w, m0[:, :, 0])
    xf, yf = ops.wavs_to_frames(noisy, clean, N, hop)
    assert _same_bits(xf, np.ascontiguousarray(data.masked_seqs_to_frames(x0, m0).T))
    assert _same_bits(yf, np.ascontiguousarray(data.masked_seqs_to_frames(y0, m0).T))
    print("pair tensors N=%d hop=%d: %d frames bitwise the composed path (error 0)" % (N, hop, xf.shape[0]))


@pytest.mark.parametrize(**_sizes(R.PAIR_SIZES))
def test_pair_logmag_tensors(ops, N, hop):
    """As test_gpu_dataset.test_logmag_tensors: padding and weights bitwise, valid bins within 4 float32 ulps of
    numpy's float32 log(1 + m) of the composed magnitude; the packed frames bitwise the tensors' valid rows."""
    noisy, clean, x0, y0, m0, _, _ = _composed(ops, N, hop, MAXLEN, True)
    x, y, w = ops.wavs_to_tensors(noisy, clean, N=N, hop=hop, maxlen=MAXLEN, transform="logmag", device=DEV)
    assert _same_bits(w, m0[:, :, 0])
    valid = m0[:, :, 0] == 1.0
    worst = 0.0
    for got, mag in ((x.cpu().numpy(), x0), (y.cpu().numpy(), y0)):
        assert np.all(got[~valid] == np.float32(-1.0))
        want = np.log(np.float32(1) + mag[valid])
        g = got[valid]
        nz = want != 0
        assert np.array_equal(g[~nz], want[~nz])
        worst = max(worst, float(_ulps(g[nz], want[nz]).max()))
    print("pair logmag N=%d hop=%d: max error %.2f ulp" % (N, hop, worst))
    assert worst <= 4.0, worst
    xl, yl = ops.wavs_to_frames(noisy, clean, N, hop, transform="logmag")
    keep = w.reshape(-1) == 1
    assert torch.equal(xl, x.reshape(-1, x.shape[2])[keep]) and torch.equal(yl, y.reshape(-1, y.shape[2])[keep])


# ---- streaming ---------------------------------------------------------------------------------------------------
from test_gpu_stream import MASK_VALUE, _run                  # noqa: E402  (helpers only)


def _stream_lengths(hop):
    return [1, hop - 1, hop, hop + 1, 3 * hop + 7, 9999, 16001]


@functools.lru_cache(maxsize=None)
def _stream_offline(N, hop, int16):
    """The whole signals of a streaming size through the ragged entry points, once, TIED TO THE ORACLE here (the
    streaming sizes (512, 64) and the existing suite's (512, 512) have no other comparison with a reference)."""
    ops = _ops()
    lens = _stream_lengths(hop)
    pcm = R.batch(lens, 5 * N + hop + int(int16), int16)
    sigs = [np.ascontiguousarray(pcm[i, :n]) for i, n in enumerate(lens)]
    x, re, im, nf = ops.stft_ragged(_t(pcm), lens, N=N, hop=hop, mask_value=MASK_VALUE)
    F = N // 2 + 1
    mask = np.random.default_rng(N + 3 * hop).random((len(lens), x.shape[1], F)).astype(np.float32)
    md = _t(mask)
    y = {crop: ops.istft_ragged(re, im, md, lens, N, hop, crop=crop) for crop in (False, True)}
    w = O.sqrt_hann(N)
    xn, rn, imn, yn = x.cpu().numpy(), re.cpu().numpy(), im.cpu().numpy(), y[False].cpu().numpy()
    e_f = e_i = 0.0
    for i, n in enumerate(lens):
        S = O.stft_mc(R.as_float(sigs[i]), N, hop, w)
        f = int(nf[i])
        e_f = max([e_f] + _forward_errors(rn[i, :f], imn[i, :f], xn[i, :f], S))
        if not int16:
            ref = R.reconstruct(S, mask[i, :f], N, hop)
            e_i = max(e_i, R.rel_err(yn[i, :ref.shape[0]], ref))
    assert e_f <= R.TOL_FWD and e_i <= R.TOL_INV, (e_f, e_i)
    return dict(sigs=sigs, lens=lens, x=x, re=re, im=im, nf=nf, mask=md, y=y, e_f=e_f, e_i=e_i)


def _stream_schedules(sigs, N, hop):
    rng = np.random.default_rng(100 * N + hop)
    return [cut_schedule(len(s), N, hop, rng) for s in sigs]


@pytest.mark.parametrize(**TYPES)
@pytest.mark.parametrize(**_sizes(R.STREAM_SIZES))
def test_streamed_frames_are_bitwise_the_offline_ones(ops, N, hop, int16):
    off = _stream_offline(N, hop, int16)
    got = _run(ops, off["sigs"], _stream_schedules(off["sigs"], N, hop), N, hop, True, None)
    for b, nf in enumerate(off["nf"]):
        nf = int(nf)
        assert got["x"][b].shape[0] == nf, b
        for k in ("x", "re", "im"):
            assert torch.equal(got[k][b], off[k][b, :nf]), (b, k)
    print("streamed frames N=%d hop=%d %s: bitwise the offline ones, which are %.3e of max|S| from the oracle"
          % (N, hop, "int16" if int16 else "float32", off["e_f"]))


@pytest.mark.parametrize("crop", [False, True], ids=["full", "crop"])
@pytest.mark.parametrize(**_sizes(R.STREAM_SIZES))
def test_streamed_samples_are_bitwise_the_offline_ones(ops, N, hop, crop):
    off = _stream_offline(N, hop, False)
    got = _run(ops, off["sigs"], _stream_schedules(off["sigs"], N, hop), N, hop, crop, off["mask"])
    n_out = ops.ragged_out_lengths(off["lens"], N, hop, crop)
    y = off["y"][crop].cpu().numpy()
    for b, n in enumerate(n_out):
        assert got["y"][b].dtype == np.float32 and got["y"][b].shape[0] == n, b
        assert np.array_equal(got["y"][b], y[b, :n]), b
    print("streamed samples N=%d hop=%d %s: bitwise the offline ones, which are %.3e of max|ref| from the oracle"
          % (N, hop, "crop" if crop else "full", off["e_i"]))
