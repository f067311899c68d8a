"""The waveform criteria on the MI355X (include/drnmf_waveloss.h): the transposed ragged inverse, the per-row losses
with their gradients and the two mask heads' backward passes for a given cotangent, each against the fp64 references
of tests/wave_loss_ref.py and, for the heads, against the fused loss heads the project already trusts; then the
models' hooks on top of them.  Every test prints the largest error it measured before it asserts."""
import numpy as np
import pytest
import torch

import wave_loss_ref as R
import lstm_ref as LR
from oracle import drnmf_oracle as O
from oracle import drnmf_torch_ref as TR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


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


# ---- istft_ragged_vjp ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crop", [False, True], ids=["full", "crop"])
@pytest.mark.parametrize("int16", [True, False], ids=["int16", "float32"])
@pytest.mark.parametrize("N,hop", R.VJP_SIZES, ids=["%dx%d" % s for s in R.VJP_SIZES])
def test_vjp_matches_the_reference_and_the_device_inverse(ops, N, hop, int16, crop):
    lens, pcm, masks, g = R.vjp_case(N, hop, int16)
    n, F = len(lens), N // 2 + 1
    idx = [2, 0, 3, 1]                                           # the gather list permuted
    nfs = [R.frames(m, N, hop) for m in lens]
    T = max(nfs) + 2
    x, re, im, nf = ops.stft_ragged(_t(pcm), lens, sig_index=idx, T=T, N=N, hop=hop)
    assert [int(v) for v in nf] == [nfs[i] for i in idx]
    n_out = [R.out_length(m, N, hop, crop) for m in lens]
    assert list(ops.ragged_out_lengths(lens, N, hop, crop)) == n_out
    gd = _t(g)
    d = ops.istft_ragged_vjp(gd, re, im, lens, N, hop, sig_index=idx, crop=crop)
    assert d.shape == (n, T, F)
    dn, ren, imn = _np(d), _np(re), _np(im)
    worst = 0.0
    for k, i in enumerate(idx):
        ref = R.vjp(ren[k, :nfs[i]], imn[k, :nfs[i]], g[i], N, hop, n_out[i])
        err = R.rel_err(dn[k, :nfs[i]], ref)
        worst = max(worst, err)
        assert np.all(dn[k, nfs[i]:] == 0.0), (i, "frames behind the row's own must be 0")
    print("vjp N=%d hop=%d %s %s: max error %.3e of max|ref|" % (N, hop, "int16" if int16 else "float32",
                                                                  "crop" if crop else "full", worst))
    assert worst <= R.TOL_FWD, worst

    # junk behind every row's length must not change a bit: other samples behind n_out in g, other values in the
    # frames of re / im at and behind a row's own
    g2, re2, im2 = gd.clone(), re.clone(), im.clone()
    for k, i in enumerate(idx):
        g2[i, n_out[i]:] = 1e30
        re2[k, nfs[i]:] = float("nan")
        im2[k, nfs[i]:] = -1e30
    d2 = ops.istft_ragged_vjp(g2, re2, im2, lens, N, hop, sig_index=idx, crop=crop)
    assert torch.equal(d, d2)

    # <g, istft_ragged(m)> = <vjp(g), m> on the device's own inverse, the sums in fp64 from the downloaded tensors
    m = np.zeros((n, T, F), np.float32)
    for k, i in enumerate(idx):
        m[k, :nfs[i]] = masks[i]
    y = _np(ops.istft_ragged(re, im, _t(m), lens, N, hop, sig_index=idx, crop=crop))
    lhs = sum(float(g[i, :n_out[i]].astype(np.float64) @ y[i, :n_out[i]]) for i in idx)
    rhs = float(np.sum(dn * m.astype(np.float64)))
    print("vjp N=%d hop=%d: <g, y> = %.9e, <d_mask, m> = %.9e, difference %.3e of them" %
          (N, hop, lhs, rhs, abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300)))
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))

    # a row alone, in a slab of its own size, gives the batch's bits
    for k, i in enumerate(idx):
        one = ops.istft_ragged_vjp(gd, re[k:k + 1, :nfs[i]].contiguous(), im[k:k + 1, :nfs[i]].contiguous(), lens, N,
                                   hop, sig_index=[i], crop=crop)
        assert torch.equal(one[0], d[k, :nfs[i]]), i


# ---- wave_loss --------------------------------------------------------------------------------------------------------
def _loss_batch():
    lens = R.LOSS_LENGTHS + [3000, 9000, 700]                    # row 4: a digitally silent reference
    rng = np.random.default_rng(17)
    width = max(lens) + 7
    ref = (0.2 * rng.standard_normal((len(lens), width))).astype(np.float32)
    est = (ref + 0.05 * rng.standard_normal(ref.shape)).astype(np.float32)
    est[6] = (0.3 * rng.standard_normal(width)).astype(np.float32)       # an estimate that has nothing of its reference
    ref[4, :lens[4]] = 0.0
    return lens, est, ref


@pytest.mark.parametrize("kind", R.KINDS)
def test_wave_loss_matches_fp64(ops, kind):
    lens, est, ref = _loss_batch()
    n = len(lens)
    loss, counted, g, sums = ops.wave_loss(_t(est), _t(ref), lens, loss=kind)
    lo, co, gn, sm = _np(loss), _np(counted), _np(g), _np(sums)
    tot, cnt, worst_l, worst_g = 0.0, 0, 0.0, 0.0
    for i, m in enumerate(lens):
        rl, rc, rg = R.wave_loss(est[i, :m], ref[i, :m], kind)
        assert co[i] == float(rc), i
        assert np.all(gn[i, m:] == 0.0), i
        if not rc:
            assert i == 4 and kind == "si_sdr" and lo[i] == 0.0 and np.all(gn[i] == 0.0)
            continue
        tot, cnt = tot + rl, cnt + 1
        el = abs(lo[i] - rl) / abs(rl)
        eg = R.rel_err(gn[i, :m], rg)
        print("wave_loss %s n=%d: loss %.6e (ref %.6e, off by %.2e), g off by %.2e of max|ref|" %
              (kind, m, lo[i], rl, el, eg))
        worst_l, worst_g = max(worst_l, el), max(worst_g, eg)
    assert worst_l <= 1e-6 and worst_g <= 1e-5, (worst_l, worst_g)
    assert sm[1] == cnt == (n if kind == "wave_mse" else n - 1)
    assert abs(sm[0] - tot) <= 1e-6 * abs(tot)
    # a row alone gives the batch's bits
    for i in (0, 3, 5):
        l1, _, g1, _ = ops.wave_loss(_t(est[i:i + 1]), _t(ref[i:i + 1]), lens[i:i + 1], loss=kind)
        assert torch.equal(l1[0], loss[i]) and torch.equal(g1[0], g[i])


# ---- head_backward_cot ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("square", [False, True], ids=["plain", "square"])
@pytest.mark.parametrize("rows", R.HEAD_ROWS)
@pytest.mark.parametrize("r,F", R.HEAD_SHAPES, ids=["r%dF%d" % s for s in R.HEAD_SHAPES])
def test_head_backward_cot(ops, r, F, rows, square):
    rng = np.random.default_rng(1000 * rows + 10 * r + F + int(square))
    hid = (rng.random((rows, 2 * r)) * (rng.random((rows, 2 * r)) < 0.5) + 0.01).astype(np.float32)
    kc = (0.3 * rng.standard_normal((r, F))).astype(np.float32)
    kn = (0.3 * rng.standard_normal((r, F))).astype(np.float32)
    hd, kcd, knd = _t(hid), _t(kc), _t(kn)
    mask, A, Bn = ops.head_forward(hd, kcd, knd, square=square, want_ab=True)
    names = ("d_hidden", "d_kernel_clean", "d_kernel_noise")

    # (i) a random cotangent in rows padded to a stride above F, against fp64 autograd of the head
    dm = rng.standard_normal((rows, F)).astype(np.float32)
    buf = torch.full((rows, F + 3), float("nan"), device=DEV)
    buf[:, :F] = _t(dm)
    got = ops.head_backward_cot(buf[:, :F], hd, kcd, knd, A, Bn, square=square)
    ref = R.head_cot_grads(hid, kc, kn, dm, square)
    errs = [R.rel_err(_np(a), b) for a, b in zip(got, ref)]
    print("head_backward_cot r=%d F=%d rows=%d square=%d: " % (r, F, rows, square) +
          ", ".join("%s %.2e" % p for p in zip(names, errs)))
    assert max(errs) <= R.G_TOL, errs

    # (ii) the MSE's own cotangent against the fused entry on the same inputs
    x = rng.random((rows, F)).astype(np.float32)
    y = rng.random((rows, F)).astype(np.float32)
    w = (rng.random(rows) < 0.8).astype(np.float32)
    xd, yd, wd = _t(x), _t(y), _t(w)
    _, fh, fkc, fkn = ops.loss_head_backward(xd, hd, kcd, knd, mask, A, Bn, yd, wd, square=square)
    dm2 = wd[:, None] * (2.0 / F) * (xd * mask - yd) * xd
    got2 = ops.head_backward_cot(dm2, hd, kcd, knd, A, Bn, square=square)
    errs2 = [R.rel_err(_np(a), _np(b)) for a, b in zip(got2, (fh, fkc, fkn))]
    print("   against drnmf_loss_head_backward: " + ", ".join("%s %.2e" % p for p in zip(names, errs2)))
    assert max(errs2) <= R.G_TOL, errs2


# ---- lstm_head_backward_cot ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,F,H", R.LSTM_HEAD_SHAPES, ids=["B%dT%dF%dH%d" % s for s in R.LSTM_HEAD_SHAPES])
def test_lstm_head_backward_cot(ops, B, T, F, H):
    K = 1
    rng = np.random.default_rng(100 * B + 10 * T + F + H)
    x, valid = LR.masked_input(rng, B, T, F)
    wt = LR.random_weights(rng, F, H, K)
    wd = [_t(a) for a in wt]
    desc = ops.make_lstm_desc(B, T, F, H, K)
    params = ops.lstm_prepare_params(desc, [wd[0]], [wd[1]], [wd[2]], wd[3], wd[4])
    ws = ops.lstm_train_workspace(desc, DEV)
    ops.lstm_train_forward(_t(x), -1.0, params, desc, ws)         # the fused head reads xm from the workspace
    xm = (x * valid[..., None]).astype(np.float32)
    hid = rng.standard_normal((B, T, H)).astype(np.float32)
    ld = ops.lstm_hidden_ld(H)
    hbuf = torch.zeros((B, T, ld), device=DEV)
    hbuf[..., :H] = _t(hid)
    names = ("d_hidden", "d_w_out", "d_b_out")

    def run(dm, hd):
        out = (torch.full((B, T, H), float("nan"), device=DEV), torch.full((H, F), float("nan"), device=DEV),
               torch.full((F,), float("nan"), device=DEV))
        ops.lstm_head_backward_cot(dm, hd, params, wd[3], desc, ws, *out)
        return out

    dm = rng.standard_normal((B, T, F)).astype(np.float32)
    ref = R.lstm_head_cot_grads(hid, wt[3], wt[4], dm)
    for lname, hd in (("contiguous", _t(hid)), ("padded", hbuf[..., :H])):
        errs = [R.rel_err(_np(a), b) for a, b in zip(run(_t(dm), hd), ref)]
        print("lstm_head_backward_cot B%dT%dF%dH%d %s: " % (B, T, F, H, lname) +
              ", ".join("%s %.2e" % p for p in zip(names, errs)))
        assert max(errs) <= R.G_TOL, errs

    # the MSE's own cotangent against the fused entry on the same inputs
    y = rng.random((B, T, F)).astype(np.float32)
    w = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=(B, T))
    w[0, 0] = 1.0
    sums = torch.empty(2, device=DEV)
    fused = (torch.empty((B, T, H), device=DEV), torch.empty((H, F), device=DEV), torch.empty((F,), device=DEV))
    ops.lstm_loss_head_backward(_t(y), _t(w), hbuf[..., :H], params, wd[3], desc, ws, sums, *fused)
    s = ops.lstm_head_forward(hbuf[..., :H], params, desc)
    xmd = _t(xm)
    dm2 = _t(w)[..., None] * (2.0 / F) * (xmd * s - _t(y)) * xmd
    errs2 = [R.rel_err(_np(a), _np(b)) for a, b in zip(run(dm2, hbuf[..., :H]), fused)]
    print("   against drnmf_lstm_loss_head_backward: " + ", ".join("%s %.2e" % p for p in zip(names, errs2)))
    assert max(errs2) <= R.G_TOL, errs2


# ---- the models' hooks -----------------------------------------------------------------------------------------------

WN, WHOP, WF = 64, 16, 33
FAMILIES = ["snmf", "lstm"]


def _wav_set(seed=3, n=6):
    """A fixed synthetic set: the generator's speech part (clean) and speech + noise (noisy) magnitudes under one
    random phase, pushed through the reference inverse; recordings of 300 .. 1500 samples, float32."""
    P = O.synth_problem(n, 100, WF, 4, seed=seed, density=0.2)
    rng = np.random.default_rng(seed)
    w = O.sqrt_hann(WN)
    lens = [300, 1500] + [int(v) for v in rng.integers(300, 1501, size=n - 2)]
    noisy, clean = [], []
    for i in range(n):
        ph = np.exp(1j * rng.uniform(-np.pi, np.pi, size=(WF, 100)))
        for mag, out in ((P["X"][i], noisy), (P["Y"][i], clean)):
            S = mag.T.astype(np.float64) * ph
            out.append(O.reconstruct(S.real, S.imag, None, WHOP, w)[:lens[i]].astype(np.float32))
    return noisy, clean, P["W"]


def _build(family, W, seed=0, lr=1e-3, compile_=True):
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


def _ref_forward(family, m, weights, x):
    """The model's mask in fp64 torch from weight tensors `weights` (get_weights order) and x [B,T,F] fp64."""
    if family == "snmf":
        names = ["log_h0"] + list(m.cell._alt.keys()) + ["kc", "kn"]
        wd = dict(zip(names, weights))
        alt = {k: wd[k] for k in m.cell._alt.keys()}
        hs = TR.cell_outputs(x, alt, m.cell.maps_from_alt.labels_per_k, 2, wd["log_h0"], -1.0)
        return TR.head_terms(x, x, torch.ones(x.shape[:2], dtype=torch.float64), hs, wd["kc"], wd["kn"])[2]
    K = 2
    hs = LR.lstm_layers(x, weights[0:3 * K:3], weights[1:3 * K:3], weights[2:3 * K:3], -1.0, "sigmoid")
    return LR.head(hs[-1], weights[3 * K], weights[3 * K + 1])


def _ref_wave(family, m, ops, noisy, clean, kind):
    """(mean loss over the counted recordings, their number, gradients of the SUM in get_weights order) by fp64
    autograd end to end: the device's own STFT rows as inputs, the model, the reference reconstruction, the loss."""
    lens = [v.shape[0] for v in noisy]
    pcm = np.zeros((len(lens), max(lens)), np.float32)
    for i, v in enumerate(noisy):
        pcm[i, :lens[i]] = v
    x, re, im, nf = ops.stft_ragged(_t(pcm), lens, N=WN, hop=WHOP, mask_value=-1.0)
    weights = [torch.tensor(a.astype(np.float64), requires_grad=True) for a in m.get_weights()]
    mask = _ref_forward(family, m, weights, x.cpu().double())
    tot, cnt = 0.0, 0
    for i, n in enumerate(lens):
        y = R.reconstruct_torch(_np(re[i, :nf[i]]), _np(im[i, :nf[i]]), mask[i, :nf[i]], WN, WHOP, n)
        s = torch.as_tensor(clean[i][:n].astype(np.float64))
        if kind == "si_sdr" and float((s * s).sum()) == 0.0:
            continue
        tot, cnt = tot + R.wave_loss_torch(y, s, kind), cnt + 1
    tot.backward()
    return float(tot.detach()) / cnt, cnt, [w.grad.numpy() if w.grad is not None else None for w in weights]


def _grad_names(family, m):
    if family == "snmf":
        names = ["log_h0"] + list(m.cell._alt.keys()) + ["kernel_clean", "kernel_noise"]
    else:
        names = [n for n, _ in m.flat_layout_items()]
    return names


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_wave_gradients_match_end_to_end_autograd(ops, family, kind):
    noisy, clean, W = _wav_set()
    m = _build(family, W)
    bank = m._wave_bank(noisy, clean, WN, WHOP, None, "test")
    x, cot_fn = m._wave_batch(bank, np.arange(len(noisy)), WN, WHOP, kind)
    flat = m.loss_and_grads_cot(x, cot_fn).clone()
    torch.cuda.synchronize()
    ref_loss, cnt, ref = _ref_wave(family, m, ops, noisy, clean, kind)
    byname = dict(zip(_grad_names(family, m), ref))
    f = _np(flat)
    print("%s %s: loss sum %.6e (ref %.6e), count %g" % (family, kind, f[-4], ref_loss * cnt, f[-3]))
    assert f[-3] == cnt == f[-2] and f[-1] == 0.0
    assert abs(f[-4] - ref_loss * cnt) <= 1e-5 * abs(ref_loss * cnt)
    checked = 0
    for n, _ in m._train_items:
        err = R.rel_err(_np(m._gview[n]), byname[n])
        print("   %s: max|d|/max|ref| = %.3e" % (n, err))
        assert err <= R.G_TOL, (n, err)
        checked += 1
    assert checked >= 4
    # test_on_wavs is the same loss without a step
    got = m.test_on_wavs(noisy, clean, loss=kind, N=WN, hop=WHOP, batch_size=4)
    assert abs(got - ref_loss) <= 1e-5 * abs(ref_loss), (got, ref_loss)


@pytest.mark.parametrize("family", FAMILIES)
def test_custom_step_fed_the_mse_cotangent_is_train_on_batch(ops, family):
    noisy, clean, W = _wav_set()
    lr = 1e-3
    a, b = _build(family, W, lr=lr), _build(family, W, lr=lr)
    P = O.synth_problem(5, 9, WF, 4, seed=11, ragged=True, density=0.2)
    x, y = _t(P["X"]), _t(P["Y"])
    w = (x != -1.0).any(-1).float()
    la = float(a.train_on_batch(x, y, w))

    def cot_fn(mask):
        xm = x * w[..., None] if family == "lstm" else x
        e = xm * mask - y
        sums = torch.stack([(w * (e * e).mean(-1)).sum(), (w != 0).float().sum()])
        return sums, w[..., None] * (2.0 / WF) * e * xm
    lb = float(b.train_on_batch_custom(x, cot_fn))
    assert abs(la - lb) <= 1e-5 * abs(la), (la, lb)
    for n, wa, wb in zip(_grad_names(family, a), a.get_weights(), b.get_weights()):
        d = float(np.max(np.abs(wa - wb)))
        print("%s %s: weights after one step differ by %.3e" % (family, n, d))
        assert d <= R.G_TOL * lr, (n, d)


@pytest.mark.parametrize("family", FAMILIES)
def test_fit_waveform_lowers_the_loss_and_repeats_bitwise(ops, family):
    noisy, clean, W = _wav_set()
    runs = []
    for _ in range(2):
        m = _build(family, W, lr=2e-3)
        before = m.test_on_wavs(noisy, clean, N=WN, hop=WHOP)
        hist = m.fit_waveform(noisy, clean, loss="si_sdr", batch_size=len(noisy), epochs=20, N=WN, hop=WHOP,
                              validation_wavs=(noisy, clean))
        after = m.test_on_wavs(noisy, clean, N=WN, hop=WHOP)
        runs.append((before, after, m.get_weights(), hist))
    before, after, _, hist = runs[0]
    print("%s: -SI-SDR %.4f dB before, %.4f dB after 20 steps on the synthetic set" % (family, before, after))
    assert after < before
    assert len(hist["loss"]) == 20 and len(hist["val_loss"]) == 20 and abs(hist["val_loss"][-1] - after) == 0.0
    for wa, wb in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(wa, wb)


def test_models_refuse_before_any_launch(ops):
    from drnmf_amd import layers
    noisy, clean, W = _wav_set()
    m = _build("snmf", W, compile_=False)
    for call in (lambda: m.train_on_wavs(noisy, clean, N=WN, hop=WHOP),
                 lambda: m.fit_waveform(noisy, clean, N=WN, hop=WHOP),
                 lambda: m.train_on_batch_custom(torch.zeros((1, 2, WF), device=DEV), None),
                 lambda: m.loss_and_grads_cot(torch.zeros((1, 2, WF), device=DEV), None)):
        with pytest.raises(ValueError, match="compile"):
            call()
    m.compile()
    with pytest.raises(ValueError, match="bins"):
        m.train_on_wavs(noisy, clean, N=128, hop=32)
    with pytest.raises(ValueError, match="bins"):
        m.test_on_wavs(noisy, clean, N=128, hop=32)
    with pytest.raises(ValueError, match="loss must be"):
        m.train_on_wavs(noisy, clean, loss="sdr", N=WN, hop=WHOP)
    lstm = layers.build_lstm(dict(mask_value=-1.0, maxseq=8, input_dim=WF, output_dim=WF, K_layers=1, hidden_dim=13,
                                  stateful=True), device=torch.device(DEV))
    lstm.compile()
    for call in (lambda: lstm.train_on_wavs(noisy, clean, N=WN, hop=WHOP),
                 lambda: lstm.test_on_wavs(noisy, clean, N=WN, hop=WHOP),
                 lambda: lstm.fit_waveform(noisy, clean, N=WN, hop=WHOP)):
        with pytest.raises(NotImplementedError, match="stateful"):
            call()
    h16 = layers.build_lstm(dict(mask_value=-1.0, maxseq=8, input_dim=WF, output_dim=WF, K_layers=1, hidden_dim=32,
                                 operand_dtype="float16"), device=torch.device(DEV))
    with pytest.raises(NotImplementedError):
        h16.compile()
    with pytest.raises(ValueError, match="compile"):
        h16.train_on_wavs(noisy, clean, N=WN, hop=WHOP)
    snmf = layers.build_snmf(dict(r=4, sparsity=0.1, cf='ed', max_iter=2, conv_eps=0., random_seed=1),
                             np.ones((WF, 8), np.float32), device=DEV)
    for call in (lambda: snmf.train_on_wavs(noisy, clean, N=WN, hop=WHOP),
                 lambda: snmf.test_on_wavs(noisy, clean, N=WN, hop=WHOP),
                 lambda: snmf.fit_waveform(noisy, clean, N=WN, hop=WHOP),
                 lambda: snmf.train_on_batch_custom(None, None)):
        with pytest.raises(NotImplementedError, match="SparseNMFModel"):
            call()
