"""The online noise-adaptive sparse-NMF baseline on the GPU (csrc/snmf_online.hip, ops.snmf_online_forward,
SparseNMFModel(adapt_noise='online')) against the fp64 numpy reference tests/snmf_online_ref.py.

Inputs: the adaptive tests' mixtures (snmf_online_ref.mixture), sparsity 0.1, 30 iterations unless said.  Bounds, as
in tests/test_gpu_snmf_adapt.py: the mask MSE is the project's MASK_MSE_TOL = 1e-8; the dictionaries are held to
max(8 e32, 1e-6) max|W64|, e32 being the relative error of the same numpy reference run in float32 on the same input
(the factor 8 covers the MFMA summation order differing from BLAS's); the divergence of every full block to 1e-4
relative.  Everything about cuts, batch position and padding is bitwise."""
import numpy as np
import pytest
import torch

import snmf_model_ref as R
import snmf_online_ref as Q

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPARSITY, MASK_VALUE = 0.1, -1.0
# (B, T, F, N, n0), L, the extra conditions
CASES = [((1, 40, 5, 10, 5), 16, {}),
         ((4, 70, 33, 48, 24), 16, dict(lengths=(70, 33, 16, 0), gone=(0, 20))),
         ((2, 100, 33, 50, 19), 32, {}),
         ((2, 200, 129, 200, 100), 64, dict(forget=0.9, w_iter=3)),
         ((1, 130, 257, 512, 256), 64, {}),
         ((2, 48, 33, 48, 0), 16, {}),
         ((2, 48, 33, 48, 48), 16, {}),
         ((2, 200, 129, 200, 100), 64, dict(power=2.0)),
         ((2, 200, 129, 200, 100), 64, dict(n_iter=200))]
IDS = ["%s-L%d%s" % ("x".join(map(str, s)), L, "".join("-%s%s" % (k, v) for k, v in sorted(e.items())
                                                      if k not in ("lengths", "gone"))) for s, L, e in CASES]


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def t(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)   # (a copy: some inputs are read-only)


def problem(shape, extra=None):
    """x (with the case's row lengths and its interior masked frame), Wn, h_init."""
    extra = extra or {}
    B, T, F, N, n0 = shape
    x, Wn, hn = Q.mixture(B, T, F, N, n0, lengths=extra.get("lengths"), mask_value=MASK_VALUE)
    if "gone" in extra:
        b, fr = extra["gone"]
        x[b, fr] = MASK_VALUE
    return x, Wn, hn


def settings(extra):
    return dict(n_iter=extra.get("n_iter", 30), w_iter=extra.get("w_iter", 1), forget=extra.get("forget", 1.0),
                power=extra.get("power", 1.0))


_REF = {}


def reference(i, dtype=np.float64):
    """(mask, H, rows) of the numpy reference for CASES[i], computed once per key and never changed."""
    key = (i, np.dtype(dtype).name)
    if key not in _REF:
        shape, L, extra = CASES[i]
        x, Wn, hn = problem(shape, extra)
        s = settings(extra)
        mask, H, rows = Q.online_forward(x, Wn.astype(np.float64), hn.astype(np.float64), SPARSITY, s["n_iter"],
                                         shape[4], L, w_iter=s["w_iter"], forget=s["forget"], power=s["power"],
                                         mask_value=MASK_VALUE, dtype=dtype)
        mask.setflags(write=False)
        H.setflags(write=False)
        _REF[key] = (mask, H, rows)
    return _REF[key]


class Run(object):
    """A state of B streams and what its calls returned."""

    def __init__(self, ops, B, F, N, n0, L, Wn, hn, n_iter=30, w_iter=1, forget=1.0, power=1.0):
        self.ops, self.hn, self.Wn = ops, t(hn), t(Wn)
        self.kw = dict(w_iter=w_iter, forget=forget, power=power, mask_value=MASK_VALUE)
        self.n_iter, self.n0 = n_iter, n0
        self.state = ops.snmf_online_state(B, F, N, n0, L, self.Wn, DEV)

    def push(self, x):
        m, H = self.ops.snmf_online_forward(t(x), self.hn, SPARSITY, self.n_iter, self.n0, self.state, return_h=True,
                                            **self.kw)
        return m.cpu().numpy(), H.cpu().numpy()

    def everything(self):
        """(W, counts, A, Bm) as numpy."""
        W, c = self.ops.snmf_online_dictionaries(self.state)
        A, Bm = self.ops.snmf_online_statistics(self.state)
        return tuple(a.cpu().numpy() for a in (W, c, A, Bm))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_the_reference(ops, i):
    shape, L, extra = CASES[i]
    B, T, F, N, n0 = shape
    x, Wn, hn = problem(shape, extra)
    s = settings(extra)
    run = Run(ops, B, F, N, n0, L, Wn, hn, **s)
    m, H = run.push(x)
    W, counts, A, Bm = run.everything()
    m64, H64, rows64 = reference(i)
    _, _, rows32 = reference(i, np.float32)
    valid = np.any(x != MASK_VALUE, axis=-1)
    assert all(np.isfinite(a).all() for a in (m, H, W, A, Bm))
    assert not m[~valid].any() and not H[~valid].any(), "masked frames must be exactly 0"
    assert counts.tolist() == valid.sum(1).tolist() == [r.count for r in rows64]
    W64 = np.stack([r.W for r in rows64])
    W32 = np.stack([r.W for r in rows32])
    mse = float(np.mean((m - m64) ** 2))
    scale = float(np.abs(W64).max())
    e32 = float(np.abs(W32 - W64).max()) / scale
    dW = float(np.abs(W - W64).max())
    print("snmf online %s: mask MSE %.3e, max|dW| %.3e (bound %.3e, e32 %.3e)"
          % (IDS[i], mse, dW, max(8 * e32, 1e-6) * scale, e32))
    assert mse <= R.MASK_MSE_TOL
    assert dW <= max(8 * e32, 1e-6) * scale
    assert np.array_equal(W[:, :, :n0], np.broadcast_to(Wn[:, :n0], (B, F, n0)))      # fixed atoms: the bits of Wn
    if n0 == N:                                                                      # the fixed baseline
        want = ops.snmf_mask_forward(t(x), t(Wn), t(hn), SPARSITY, s["n_iter"], power=s["power"],
                                     mask_value=MASK_VALUE).cpu().numpy()
        assert np.abs(m - want).max() <= 1e-5
        assert np.array_equal(W, np.broadcast_to(Wn, W.shape)) and A.size == 0
    # block by block, every row as a stream of its own over its valid frames: the divergence of each full block
    # against the reference's, and the same bits as the one call above
    for b in range(B):
        xv = x[b][valid[b]]
        if valid[b].sum() < L:
            assert np.array_equal(W[b], Wn)                              # no block filled: no update
        one = Run(ops, 1, F, N, n0, L, Wn, hn, **s)
        for k, (Vb, Hb, Wk64) in enumerate(rows64[b].blocks):
            Wk = one.everything()[0][0]
            mk, Hk = one.push(xv[None, k * L:(k + 1) * L])
            assert np.array_equal(mk[0], m[b][valid[b]][k * L:(k + 1) * L]), (b, k)
            assert np.array_equal(Hk[0], H[b][valid[b]][k * L:(k + 1) * L]), (b, k)
            d, d64 = Q.divergence(Vb, Wk, Hk[0]), Q.divergence(Vb, Wk64, Hb)
            print("  row %d block %d: divergence %.6e, reference %.6e" % (b, k, d, d64))
            assert abs(d - d64) <= 1e-4 * d64
            if n0 < N and k:
                assert np.abs(np.sqrt((Wk[:, n0:].astype(np.float64) ** 2).sum(0)) - 1).max() <= 1e-6


# ---- bitwise: cuts, batch position, padding, reset --------------------------------------------------------------
SHAPE_B, L_B = (3, 116, 33, 48, 24), 16
PUSHES = (1, 15, 16, 17, 3, 64, 0)


@pytest.fixture(scope="module")
def whole(ops):
    """The three rows of SHAPE_B in one call: (x, Wn, hn, mask, H, (W, counts, A, Bm))."""
    B, T, F, N, n0 = SHAPE_B
    x, Wn, hn = problem(SHAPE_B)
    run = Run(ops, B, F, N, n0, L_B, Wn, hn, w_iter=2, forget=0.9)
    m, H = run.push(x)
    out = (x, Wn, hn, m, H, run.everything())
    for a in (x, m, H) + out[5]:
        a.setflags(write=False)
    return out


def _new_run(ops, B, Wn, hn):
    _, _, F, N, n0 = SHAPE_B
    return Run(ops, B, F, N, n0, L_B, Wn, hn, w_iter=2, forget=0.9)


def test_pushes_equal_the_whole_row(ops, whole):
    """Pushes of 1, 15, 16, 17, 3, 64 and 0 frames, every row of the batch with that schedule rotated (so the rows sit at
    different phases of their blocks in every call, a row with fewer frames padded with masked ones), and one call
    without frames at all."""
    x, Wn, hn, m, H, state = whole
    B, T, F, N, n0 = SHAPE_B
    assert sum(PUSHES) == T
    sched = [PUSHES[b * 2:] + PUSHES[:b * 2] for b in range(B)]
    run = _new_run(ops, B, Wn, hn)
    at = [0] * B
    got_m, got_H = [[] for _ in range(B)], [[] for _ in range(B)]
    for k in range(len(PUSHES)):
        ns = [sched[b][k] for b in range(B)]
        Tk = max(ns)
        xk = np.full((B, Tk, F), MASK_VALUE, np.float32)
        for b in range(B):
            xk[b, :ns[b]] = x[b, at[b]:at[b] + ns[b]]
        mk, Hk = run.push(xk)
        for b in range(B):
            assert not mk[b, ns[b]:].any() and not Hk[b, ns[b]:].any()
            got_m[b].append(mk[b, :ns[b]])
            got_H[b].append(Hk[b, :ns[b]])
            at[b] += ns[b]
        if k == 2:
            m0, H0 = run.push(np.zeros((B, 0, F), np.float32))
            assert m0.shape == (B, 0, F) and H0.shape == (B, 0, N)
    assert at == [T] * B
    for b in range(B):
        assert np.array_equal(np.concatenate(got_m[b]), m[b]), b
        assert np.array_equal(np.concatenate(got_H[b]), H[b]), b
    for a, w, what in zip(run.everything(), state, ("dictionaries", "counts", "A", "Bm")):
        assert np.array_equal(a, w), what
    assert state[1].tolist() == [T] * B
    assert np.abs(state[0][:, :, n0:] - Wn[:, n0:]).max() > 1e-3         # the noise atoms did move


def test_rows_do_not_depend_on_batch_size_position_or_padding(ops, whole):
    x, Wn, hn, m, H, state = whole
    B, T, F, N, n0 = SHAPE_B
    for b in range(B):
        run = _new_run(ops, 1, Wn, hn)
        mb, Hb = run.push(x[b:b + 1])
        assert np.array_equal(mb[0], m[b]) and np.array_equal(Hb[0], H[b]), b
        for a, w in zip(run.everything(), state):
            assert np.array_equal(a[0], w[b]), b
    order = [2, 0, 1]
    run = _new_run(ops, B, Wn, hn)
    mo, Ho = run.push(x[order])
    assert np.array_equal(mo, m[order]) and np.array_equal(Ho, H[order])
    for a, w in zip(run.everything(), state):
        assert np.array_equal(a, w[order])
    xp = np.full((B + 1, T + 27, F), MASK_VALUE, np.float32)             # T padded, a silent row beside them
    xp[:B, :T] = x
    xp[B, :40] = 0.0
    run = _new_run(ops, B + 1, Wn, hn)
    mp, Hp = run.push(xp)
    assert np.array_equal(mp[:B, :T], m) and np.array_equal(Hp[:B, :T], H)
    assert not mp[:, T:].any() and not Hp[:, T:].any()
    W, counts, A, Bm = run.everything()
    for a, w in zip((W[:B], counts[:B], A[:B], Bm[:B]), state):
        assert np.array_equal(a, w)
    # the silent row is valid: it fills two blocks of zeros, whose update the guard holds back
    assert counts[B] == 40 and np.array_equal(W[B], Wn) and not A[B].any() and not mp[B].any()
    assert np.array_equal(W[:, :, :n0], np.broadcast_to(Wn[:, :n0], (B + 1, F, n0)))


def test_reset_repeats_the_first_run_and_one_stream_can_restart(ops, whole):
    x, Wn, hn, m, H, state = whole
    B, T, F, N, n0 = SHAPE_B
    run = _new_run(ops, B, Wn, hn)
    run.push(x[:, :50])
    ops.snmf_online_reset(run.state, run.Wn)
    W, counts, A, Bm = run.everything()
    assert np.array_equal(W, np.broadcast_to(Wn, W.shape)) and not counts.any() and not A.any() and not Bm.any()
    mr, Hr = run.push(x)
    assert np.array_equal(mr, m) and np.array_equal(Hr, H)
    for a, w in zip(run.everything(), state):
        assert np.array_equal(a, w)
    # row 1 alone starts over after 50 frames; rows 0 and 2 go on
    run = _new_run(ops, B, Wn, hn)
    run.push(x[:, :50])
    ops.snmf_online_reset(run.state, run.Wn, rows=[False, True, False])
    x2 = x[:, 50:].copy()
    x2[1] = x[1, :T - 50]
    m2, _ = run.push(x2)
    assert np.array_equal(m2[0], m[0, 50:]) and np.array_equal(m2[2], m[2, 50:])
    assert np.array_equal(m2[1], m[1, :T - 50])
    assert run.everything()[1].tolist() == [T, T - 50, T]


def test_the_first_block_is_the_fixed_model(ops, whole):
    x, Wn, hn, m, _, _ = whole
    want = ops.snmf_mask_forward(t(x[:, :L_B]), t(Wn), t(hn), SPARSITY, 30, mask_value=MASK_VALUE).cpu().numpy()
    assert np.abs(m[:, :L_B] - want).max() <= 1e-5
    later = ops.snmf_mask_forward(t(x[:, L_B:]), t(Wn), t(hn), SPARSITY, 30, mask_value=MASK_VALUE).cpu().numpy()
    assert np.abs(m[:, L_B:] - later).max() > 1e-3                       # ... and the later ones are not


# ---- the model ---------------------------------------------------------------------------------------------------
N_M, HOP_M, F_M = 256, 64, 129


def _model(adapt="online", **kw):
    from drnmf_amd import layers
    rng = np.random.RandomState(4)
    W = (rng.rand(F_M, 200) + 0.05).astype(np.float32)
    return layers.SparseNMFModel(W, 100, SPARSITY, n_iter=30, h_init=rng.rand(200), device=DEV, adapt_noise=adapt,
                                 **kw)


def _recordings():
    rng = np.random.default_rng(5)
    return [(rng.standard_normal(n) * 3000 * (1 + 0.5 * np.sin(np.arange(n) / 700.0))).astype(np.int16)
            for n in (3000, 4517, 2400)]


def test_model_forward_is_the_op_and_carries_the_state(ops):
    m = _model(adapt_block=32, adapt_forget=0.9, adapt_w_iter=2)
    before = m.get_weights()[0].copy()
    x = t(problem((2, 100, 129, 200, 100))[0])
    Wn, hn = m._operands()
    state = ops.snmf_online_state(2, F_M, 200, 100, 32, Wn, DEV)
    want = [ops.snmf_online_forward(p, hn, SPARSITY, 30, 100, state, w_iter=2, forget=0.9, mask_value=MASK_VALUE)
            for p in (x[:, :41], x[:, 41:])]
    m.reset_states(batch_size=2)
    assert torch.equal(m.forward(x[:, :41]), want[0])
    got, Wd = m.forward(x[:, 41:], return_dictionaries=True)             # the state came along
    assert torch.equal(got, want[1])
    Ww, cw = ops.snmf_online_dictionaries(state)
    Wm, cm = m.dictionaries()
    assert torch.equal(Wm, Ww) and torch.equal(Wd, Ww) and cm.tolist() == cw.tolist() == [100, 100]
    assert tuple(Wm.shape) == (2, F_M, 200) and float((Wm[:, :, 100:] - Wn[:, 100:]).abs().max()) > 1e-3
    assert np.array_equal(m.get_weights()[0], before)                    # the stored dictionary is never modified
    with pytest.raises(ValueError, match="batch_size"):
        m.forward(x[:1])
    m.reset_states()
    assert torch.equal(m.forward(x[:, :41]), want[0])
    # predict_on_batch carries the state as forward does
    m.reset_states(batch_size=2)
    xn = x.cpu().numpy()
    p1, p2 = m.predict_on_batch(xn[:, :41]), m.predict_on_batch(xn[:, 41:])
    assert np.array_equal(p1, want[0].cpu().numpy()) and np.array_equal(p2, want[1].cpu().numpy())
    # a changed stored dictionary rebuilds the state
    assert m.dictionaries()[1].tolist() == [100, 100]
    m.set_weights([before[:, ::-1].copy()])
    Wm, cm = m.dictionaries()
    assert cm.tolist() == [0, 0] and torch.equal(Wm[1], m._operands()[0]) and not torch.equal(Wm[1], Wn)
    m.forward(x[:, :5])
    assert m.dictionaries()[1].tolist() == [5, 5]
    with pytest.raises(NotImplementedError, match="stateful"):
        m.enhance(_recordings(), N=N_M, hop=HOP_M)


def test_stream_equals_the_whole_recordings(ops):
    """model.stream pushed with odd chunk sizes on 3 recordings of unequal length against stft_ragged -> forward ->
    istft_ragged after a reset: the float32 samples bit for bit."""
    m = _model(adapt_block=16)
    wavs = _recordings()
    lens = [len(w) for w in wavs]
    pcm = np.zeros((len(wavs), max(lens)), np.int16)
    for i, w in enumerate(wavs):
        pcm[i, :len(w)] = w
    x, re, im, nf = ops.stft_ragged(t(pcm), lens, N=N_M, hop=HOP_M, mask_value=MASK_VALUE)
    m.reset_states(batch_size=3)
    mask = m.forward(x)
    want = ops.istft_ragged(re, im, mask, lens, N_M, HOP_M, crop=True).cpu().numpy()
    counts = m.dictionaries()[1].tolist()
    assert counts == [int(n) for n in nf] and min(counts) >= 2 * 16      # every stream adapted at least twice
    fixed = _model(adapt=False).forward(x)
    assert float((mask - fixed).abs().max()) > 1e-3                      # (else the comparison below shows nothing)
    st = m.stream(3, N=N_M, hop=HOP_M, dtype="float32", crop=True)
    for sizes in ((97, 1, 333, 0, 64, 1001, 257), (4517,)):
        st.reset()
        at, out = [0] * 3, [[] for _ in range(3)]
        k = 0
        while any(at[b] < lens[b] for b in range(3)):
            chunks = []
            for b in range(3):
                n = sizes[(k + b) % len(sizes)]
                chunks.append(wavs[b][at[b]:at[b] + n])
                at[b] += n
            for b, y in enumerate(st.push(chunks)):
                out[b].append(y)
            k += 1
        for b, y in enumerate(st.close()):
            out[b].append(y)
        for b, n in enumerate(lens):
            y = np.concatenate(out[b])
            assert y.shape == (n,) and np.array_equal(y, want[b, :n]), (sizes, b)
        assert m.dictionaries()[1].tolist() == counts


def test_val_loss_resets_and_runs_one_row_per_recording(ops):
    m = _model(adapt_block=16)
    wavs = _recordings()
    clean = [(0.8 * w).astype(np.int16) for w in wavs]
    first = m.val_loss(wavs, clean, N=N_M, hop=HOP_M)
    assert m.dictionaries()[0].shape[0] == 3 and np.isfinite(first) and first > 0
    assert m.val_loss(wavs, clean, N=N_M, hop=HOP_M) == first            # reset in front: the same number again
