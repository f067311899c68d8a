"""The streaming path on the MI355X (include/drnmf_stream.h): frames and samples collected over arbitrary cut
schedules are BITWISE those of ops.stft_ragged / ops.istft_ragged on the whole signals (the frame bodies are the
same and a carried partial sum is continued in ascending frame order -- a derived property, not a tolerance), the
int16 output, and model.stream of both families against the same stateful model run on the whole batch."""
import functools

import numpy as np
import pytest
import torch

from test_stream_host import SIZES, cut_schedule, lengths

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MASK_VALUE = -1.0


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _ops():
    from drnmf_amd import ops
    return ops


def _signals(N, hop, int16):
    """Seven streams of the seven lengths (noise as test_gpu_enhance._batch); for N = 64 an eighth of 3 hop + 7
    samples, which is fed one sample per push."""
    lens = lengths(hop) + ([3 * hop + 7] if N == 64 else [])
    rng = np.random.default_rng(N + int(int16))
    if int16:
        return [rng.integers(-20000, 20000, size=n).astype(np.int16) for n in lens]
    return [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lens]


def _schedules(sigs, N, hop, seed):
    rng = np.random.default_rng(seed)
    sch = [cut_schedule(len(s), N, hop, rng) for s in sigs]
    if len(sigs) == 8:
        sch[7] = [1] * len(sigs[7])
    return sch


@functools.lru_cache(maxsize=None)
def _offline(N, hop, int16):
    """The whole signals through the ragged entry points, once per size: frames, a fixed random mask, and the
    masked inverse for both crops."""
    ops = _ops()
    sigs = _signals(N, hop, int16)
    lens = [len(s) for s in sigs]
    pcm = np.zeros((len(sigs), max(lens) + 1), dtype=sigs[0].dtype)
    for i, s in enumerate(sigs):
        pcm[i, :len(s)] = s
    x, re, im, nf = ops.stft_ragged(torch.from_numpy(pcm).to(DEV), lens, N=N, hop=hop, mask_value=MASK_VALUE)
    mask = torch.from_numpy(np.random.default_rng(N).random(tuple(x.shape)).astype(np.float32)).to(DEV)
    y = {crop: ops.istft_ragged(re, im, mask, lens, N, hop, crop=crop) for crop in (False, True)}
    return dict(sigs=sigs, lens=lens, x=x, re=re, im=im, nf=nf, mask=mask, y=y)


def _run(ops, sigs, schedules, N, hop, crop, mask, out_dtype="float32"):
    """Feed every stream its schedule (even streams close with their last chunk, odd ones with an empty push
    behind it) and collect frames and samples.  mask [B, >= frames, F] is sliced per push (None: no mask)."""
    B, F = len(sigs), N // 2 + 1
    ws = ops.WaveStream(B, N, hop, mask_value=MASK_VALUE, device=DEV, crop=crop)
    pos, step, fpos = [0] * B, [0] * B, [0] * B
    X, RE, IM, Y = ([[] for _ in range(B)] for _ in range(4))
    empty = np.zeros(0, dtype=sigs[0].dtype)
    for push in range(max(len(s) + (b % 2) for b, s in enumerate(schedules))):
        chunks, final = [], []
        for b in range(B):
            if step[b] < len(schedules[b]):
                c = schedules[b][step[b]]
                chunks.append(sigs[b][pos[b]:pos[b] + c])
                pos[b] += c
                step[b] += 1
                final.append(b % 2 == 0 and step[b] == len(schedules[b]))
            else:
                chunks.append(empty)
                final.append(True)
        x, re, im, n_new = ws.analyse(chunks, final=final)
        T = x.shape[1]
        assert T == int(n_new.max())
        if T == 0:
            continue
        m = None
        if mask is not None:
            m = torch.zeros((B, T, F), dtype=torch.float32, device=DEV)
        for b in range(B):
            n = int(n_new[b])
            assert bool((x[b, n:] == MASK_VALUE).all())                  # padding rows hold the mask value
            X[b].append(x[b, :n].clone())
            RE[b].append(re[b, :n].clone())
            IM[b].append(im[b, :n].clone())
            if m is not None:
                m[b, :n] = mask[b, fpos[b]:fpos[b] + n]
            fpos[b] += n
        y = ws.synthesise(re, im, m, dtype=out_dtype)
        for b in range(B):
            Y[b].append(y[b])
    assert bool(ws.closed.all()) and pos == [len(s) for s in sigs]
    cat = lambda rows: [torch.cat(r) for r in rows]
    return dict(x=cat(X), re=cat(RE), im=cat(IM), y=[np.concatenate(r) for r in Y], ws=ws)


@functools.lru_cache(maxsize=None)
def _streamed(N, hop, int16, crop, seed):
    off = _offline(N, hop, int16)
    return _run(_ops(), off["sigs"], _schedules(off["sigs"], N, hop, seed), N, hop, crop, off["mask"])


@pytest.mark.parametrize("int16", [True, False], ids=["int16", "float32"])
@pytest.mark.parametrize("N,hop", SIZES)
def test_forward_frames_are_bitwise_the_offline_ones(ops, N, hop, int16):
    off, got = _offline(N, hop, int16), _streamed(N, hop, int16, True, 1)
    for b, nf in enumerate(off["nf"]):
        nf = int(nf)
        assert got["x"][b].shape[0] == nf, b
        for k in ("x", "re", "im"):
            assert torch.equal(got[k][b], off[k][b, :nf]), (b, k)


@pytest.mark.parametrize("crop", [False, True], ids=["full", "crop"])
@pytest.mark.parametrize("N,hop", SIZES)
def test_inverse_samples_are_bitwise_the_offline_ones(ops, N, hop, crop):
    off, got = _offline(N, hop, False), _streamed(N, hop, False, crop, 1)
    n_out = ops.ragged_out_lengths(off["lens"], N, hop, crop)
    y = off["y"][crop].cpu().numpy()
    for b, n in enumerate(n_out):
        assert got["y"][b].dtype == np.float32 and got["y"][b].shape[0] == n, b
        assert np.array_equal(got["y"][b], y[b, :n]), b


@pytest.mark.parametrize("N,hop", SIZES)
def test_output_does_not_depend_on_the_cuts_or_the_neighbours(ops, N, hop):
    off, a, c = _offline(N, hop, False), _streamed(N, hop, False, True, 1), _streamed(N, hop, False, True, 2)
    assert _schedules(off["sigs"], N, hop, 1) != _schedules(off["sigs"], N, hop, 2)
    for b in range(len(off["sigs"])):
        assert np.array_equal(a["y"][b], c["y"][b]), b
        for k in ("x", "re", "im"):
            assert torch.equal(a[k][b], c[k][b]), (b, k)
    b = 4                                                     # 3 hop + 7 samples, alone at B = 1
    alone = _run(ops, [off["sigs"][b]], [_schedules(off["sigs"], N, hop, 1)[b]], N, hop, True,
                 off["mask"][b:b + 1])
    assert np.array_equal(alone["y"][0], a["y"][b])
    for k in ("x", "re", "im"):
        assert torch.equal(alone[k][0], a[k][b]), k


@pytest.mark.parametrize("N,hop", SIZES)
def test_int16_output(ops, N, hop):
    """The mask here is HALF the fixed one (still in [0, 1]), at every size: istft_noDiv's gain is 2 / (N / hop),
    which is 2 at hop = N, where the squared window also peaks at 1 without a neighbour to share with -- noise of
    amplitude 0.3 under a mask up to 1 then reaches 2 * 0.3 * 4 sigma > 1 (1.20 was seen), and the comparison with
    util.wavwrite's conversion is only defined below its peak normalisation."""
    off = _offline(N, hop, False)
    n_out = ops.ragged_out_lengths(off["lens"], N, hop, True)
    mask = off["mask"] * 0.5
    y = ops.istft_ragged(off["re"], off["im"], mask, off["lens"], N, hop, crop=True)
    assert float(y.abs().max()) <= 1.0                        # below the peak util.wavwrite would divide by
    q = ops.to_int16_wav_rows(y, n_out).cpu().numpy()
    got = _run(ops, off["sigs"], _schedules(off["sigs"], N, hop, 3), N, hop, True, mask, out_dtype="int16")
    for b, n in enumerate(n_out):
        assert got["y"][b].dtype == np.int16
        assert got["y"][b].tobytes() == q[b, :n].tobytes(), b
    # samples beyond +-1 saturate and are not normalised
    rng = np.random.default_rng(7)
    loud = (3.0 * rng.standard_normal(5 * hop + 3)).astype(np.float32)
    sch = [cut_schedule(len(loud), N, hop, rng)]
    yf = _run(ops, [loud], sch, N, hop, True, None)["y"][0]
    yq = _run(ops, [loud], sch, N, hop, True, None, out_dtype="int16")["y"][0]
    assert np.max(np.abs(yf)) > 2.0
    want = np.clip(yf * np.float32(32767.0), np.float32(-32767.0), np.float32(32767.0)).astype(np.int16)
    assert np.array_equal(yq, want)
    assert yq.max() == 32767 and yq.min() == -32767


# ---- model.stream ------------------------------------------------------------------------------------------------
N_E, HOP_E, F_E = 512, 128, 257


def _model(family, stateful=True):
    from drnmf_amd import layers
    from oracle import drnmf_oracle as O
    if family == "snmf":
        r, K = 16, 3
        P = O.synth_problem(2, 4, F_E, r, seed=3)
        params = dict(input_dim=F_E, hidden_dim=2 * r, output_dim=F_E, mask_value=-1., maxseq=200, K_layers=K,
                      W=P["W"], alph=2 * r / 4.0, lam1=0.3, params_untied=["log_D", "log_alph"],
                      params_trainable=["log_D", "log_alph"])
        model = layers.build_unfolded_snmf(params, device=DEV)
        model.cell.stateful = stateful
        return model
    torch.manual_seed(0)
    np.random.seed(0)
    return layers.build_lstm(dict(mask_value=-1., maxseq=200, input_dim=F_E, output_dim=F_E, K_layers=2,
                                  hidden_dim=48, stateful=stateful), device=DEV)


def _recordings():
    rng = np.random.default_rng(4)
    lens = rng.integers(int(0.3 * 16000), int(1.5 * 16000), size=5)
    return [(rng.standard_normal(n) * 3000 * (1 + 0.5 * np.sin(np.arange(n) / 900.0))).astype(np.int16)
            for n in lens]


def _push_all(stream, wavs, schedules):
    """Feed the schedules (a stream whose schedule has run out gets empty chunks), then close()."""
    B = len(wavs)
    pos, out = [0] * B, [[] for _ in range(B)]
    for step in range(max(len(s) for s in schedules)):
        chunks = []
        for b in range(B):
            c = schedules[b][step] if step < len(schedules[b]) else 0
            chunks.append(wavs[b][pos[b]:pos[b] + c])
            pos[b] += c
        for b, y in enumerate(stream.push(chunks)):
            out[b].append(y)
    assert pos == [len(w) for w in wavs]
    for b, y in enumerate(stream.close()):
        out[b].append(y)
    return [np.concatenate(o) for o in out]


def _model_schedules(wavs):
    rng = np.random.default_rng(11)
    ten_ms = [[160] * (len(w) // 160) + ([len(w) % 160] if len(w) % 160 else []) for w in wavs]
    whole = [[len(w)] for w in wavs]
    ragged = []
    for w in wavs:                                            # some empty chunks, some below one hop
        cuts, left = [], len(w)
        while left > 0:
            c = min(int(rng.choice([0, 0, 1, 100, 128, 1000, 3333])), left)
            cuts.append(c)
            left -= c
        ragged.append(cuts)
    return dict(ten_ms=ten_ms, whole=whole, ragged=ragged)


@pytest.mark.parametrize("family", ["snmf", "lstm"])
def test_model_stream_equals_the_whole_run(ops, family):
    """model.stream under three cut schedules (10 ms pushes; one push and close(); ragged cuts with empty chunks:
    a row without new frames must keep its state) against the same stateful model, reset, run on the whole padded
    batch: ops.stft_ragged, predict_on_batch, ops.istft_ragged.  Bounds: 1e-4 of the stream's peak and 5 int16
    steps, what the project asserts for these models between batch shapes."""
    model = _model(family)
    wavs = _recordings()
    lens = [len(w) for w in wavs]
    pcm = np.zeros((len(wavs), max(lens)), np.int16)
    for i, w in enumerate(wavs):
        pcm[i, :len(w)] = w
    model.reset_states(batch_size=len(wavs))
    x, re, im, nf = ops.stft_ragged(torch.from_numpy(pcm).to(DEV), lens, N=N_E, hop=HOP_E, mask_value=-1.0)
    mask = torch.from_numpy(model.predict_on_batch(x.cpu().numpy())).to(DEV)
    y_ref = ops.istft_ragged(re, im, mask, lens, N_E, HOP_E, crop=True)
    assert float(y_ref.abs().max()) <= 1.0
    q_ref = ops.to_int16_wav_rows(y_ref, lens).cpu().numpy()
    y_ref = y_ref.cpu().numpy()
    refs = [("whole run", [y_ref[i, :n] for i, n in enumerate(lens)], [q_ref[i, :n] for i, n in enumerate(lens)])]
    if family == "lstm":                                      # a twin that is not stateful: zero state either way
        twin = _model(family, stateful=False)
        twin.set_weights(model.get_weights())
        refs.append(("enhance", twin.enhance(wavs, N=N_E, hop=HOP_E, dtype="float32", crop=True), None))
    for name, sch in _model_schedules(wavs).items():
        yf = _push_all(model.stream(len(wavs), N=N_E, hop=HOP_E, dtype="float32", crop=True), wavs, sch)
        yq = _push_all(model.stream(len(wavs), N=N_E, hop=HOP_E, dtype="int16", crop=True), wavs, sch)
        for what, rf, rq in refs:
            df = max(float(np.max(np.abs(yf[i] - rf[i])) / np.max(np.abs(rf[i]))) for i in range(len(wavs)))
            dq = None if rq is None else \
                max(int(np.max(np.abs(yq[i].astype(np.int32) - rq[i].astype(np.int32)))) for i in range(len(wavs)))
            print("stream %s %s vs %s: float32 %.3e of the peak, int16 %s" % (family, name, what, df, dq))
            for i, n in enumerate(lens):
                assert yf[i].shape == (n,) and yq[i].shape == (n,)
            assert df <= 1e-4, (name, what, df)
            assert dq is None or dq <= 5, (name, what, dq)


def test_stream_lifecycle(ops):
    model = _model("snmf")
    wavs = _recordings()[:2]
    st = model.stream(2, N=N_E, hop=HOP_E)
    sch = [[1000, 0, 2500], [77, 3000, 1]]
    feed = lambda: [st.push([wavs[b][sum(sch[b][:k]):sum(sch[b][:k + 1])] for b in range(2)]) for k in range(3)] + \
        [st.close()]
    first = feed()
    assert bool(st.closed.all())
    with pytest.raises(ValueError, match="closed"):
        st.push([wavs[0][:10], wavs[1][:0]])
    assert all(len(y) == 0 for y in st.push([wavs[0][:0], wavs[1][:0]]))      # empty chunks are still taken
    st.reset()
    assert not bool(st.closed.any())
    again = feed()
    for a, c in zip(first, again):
        for b in range(2):
            assert np.array_equal(a[b], c[b])
    st.reset()
    with pytest.raises(ValueError):
        st.push([wavs[0][:100]])                              # one chunk for two streams
    with pytest.raises(ValueError):
        st.push([wavs[0][:100], wavs[1][:100].astype(np.float32)])           # mixed types
    with pytest.raises(ValueError):
        st.push([wavs[0][:100].astype(np.float64), wavs[1][:100].astype(np.float64)])
    model.mask_value = None                                   # a model without a Masking layer
    try:
        with pytest.raises(ValueError, match="equal chunk lengths"):
            st.push([wavs[0][:100], wavs[1][:200]])
    finally:
        model.mask_value = -1.0
    with pytest.raises(ValueError, match="stateful=True"):
        _model("lstm", stateful=False).stream(2)
