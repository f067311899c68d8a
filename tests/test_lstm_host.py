"""CPU-side tests of the LSTM baseline (build_lstm, enhance.py:321-345): the fp64 reference of the contract
against torch.nn.LSTM, the Keras structure of the model, the C ABI of include/drnmf_lstm.h and its argument
validation (no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import lstm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_lstm.h")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


def test_reference_equals_torch_nn_lstm():
    """Sigmoid gates, unpadded sequences: the reference restatement equals torch.nn.LSTM with weight_ih =
    kernel^T, weight_hh = recurrent_kernel^T, bias_ih = bias, bias_hh = 0 -- an independent implementation
    that shares Keras' gate order i, f, c(g), o."""
    rng = np.random.default_rng(0)
    B, T, F, H, K = 3, 11, 7, 5, 3
    w = R.random_weights(rng, F, H, K, scale=2.0)
    x = rng.standard_normal((B, T, F))
    hs = R.lstm_layers(x, w[0:3 * K:3], w[1:3 * K:3], w[2:3 * K:3], mask_value=None,
                       recurrent_activation="sigmoid")
    net = torch.nn.LSTM(F, H, num_layers=K, batch_first=True).double()
    with torch.no_grad():
        for k in range(K):
            getattr(net, "weight_ih_l%d" % k).copy_(torch.from_numpy(w[3 * k].T.astype(np.float64)))
            getattr(net, "weight_hh_l%d" % k).copy_(torch.from_numpy(w[3 * k + 1].T.astype(np.float64)))
            getattr(net, "bias_ih_l%d" % k).copy_(torch.from_numpy(w[3 * k + 2].astype(np.float64)))
            getattr(net, "bias_hh_l%d" % k).zero_()
        ref, _ = net(torch.from_numpy(x))
    assert float((hs[-1] - ref).abs().max()) <= 1e-12


@pytest.mark.parametrize("act", ["hard_sigmoid", "sigmoid"])
def test_reference_padding_repeats_the_last_output(act):
    rng = np.random.default_rng(1)
    T, F, H, K = 9, 6, 4, 2
    w = R.random_weights(rng, F, H, K, scale=2.0)
    ks, rs, bs = w[0:3 * K:3], w[1:3 * K:3], w[2:3 * K:3]
    x = rng.random((1, 5, F))
    full = R.lstm_layers(x, ks, rs, bs, -1.0, act)[-1][0]
    xp = np.concatenate([x, -np.ones((1, T - 5, F))], axis=1)
    padded = R.lstm_layers(xp, ks, rs, bs, -1.0, act)[-1][0]
    assert torch.equal(padded[:5], full)
    for t in range(5, T):
        assert torch.equal(padded[t], full[4])
    empty = R.lstm_layers(-np.ones((1, 3, F)), ks, rs, bs, -1.0, act)[-1]
    assert float(empty.abs().max()) == 0.0


def _torch_lstm(w, K):
    F, H = w[0].shape[0], w[1].shape[0]
    net = torch.nn.LSTM(F, H, num_layers=K, batch_first=True).double()
    with torch.no_grad():
        for k in range(K):
            getattr(net, "weight_ih_l%d" % k).copy_(torch.from_numpy(w[3 * k].T.astype(np.float64)))
            getattr(net, "weight_hh_l%d" % k).copy_(torch.from_numpy(w[3 * k + 1].T.astype(np.float64)))
            getattr(net, "bias_ih_l%d" % k).copy_(torch.from_numpy(w[3 * k + 2].astype(np.float64)))
            getattr(net, "bias_hh_l%d" % k).zero_()
    return net


def test_masked_input_patterns():
    """masked_input builds what it says: the validity it reports is keras Masking's, the masked runs sit where
    the pattern puts them, and a partly masked frame (every bin but one = mask_value) is valid."""
    for mv in (-1.0, 0.0):
        x, valid = R.masked_input(np.random.default_rng(2), 14, 40, 9, "mixed", mv)
        np.testing.assert_array_equal(R.valid_frames(x, mv).numpy(), valid)
        kinds = [R.MASK_PATTERNS[b % len(R.MASK_PATTERNS)] for b in range(14)]
        for b, kind in enumerate(kinds):
            v = valid[b]
            first, last = (np.nonzero(v)[0][[0, -1]] if v.any() else (None, None))
            assert (kind == "all") == (not v.any())
            assert (kind in ("leading", "combo")) == (v.any() and first > 0)
            assert (kind in ("trailing", "combo")) == (v.any() and last < 39)
            interior = v.any() and not v[first:last + 1].all()
            assert (kind in ("interior", "combo")) == interior, kind
            nmask = (x[b] == np.float32(mv)).sum(-1)
            partial = v & (nmask == 8)
            assert (kind in ("partial", "combo")) == bool(partial.any()), kind
            assert not np.any(x[b][partial][:, 0] != np.float32(mv))       # the surviving bin is not bin 0


@pytest.mark.parametrize("mask_value", [-1.0, 0.0])
@pytest.mark.parametrize("K", [1, 3])
def test_reference_masking_equals_torch_lstm_on_the_valid_frames(K, mask_value):
    """Masking semantics of the reference against a second implementation that shares none of its masking
    logic: torch.nn.LSTM (sigmoid gates) run on each sequence's valid frames only, compacted.  The reference's
    frames at valid positions are those outputs; a masked frame repeats the last valid output, or is zero before
    the first valid frame -- in every layer (K = 3: the layers below carry their states across the gaps too)."""
    rng = np.random.default_rng(10 + K)
    B, T, F, H = 14, 23, 7, 5
    w = R.random_weights(rng, F, H, K, scale=2.0)
    x, valid = R.masked_input(rng, B, T, F, "mixed", mask_value)
    hs = R.lstm_layers(x, w[0:3 * K:3], w[1:3 * K:3], w[2:3 * K:3], mask_value, "sigmoid")[-1]
    net = _torch_lstm(w, K)
    for b in range(B):
        idx = np.nonzero(valid[b])[0]
        if len(idx):
            with torch.no_grad():
                comp, _ = net(torch.from_numpy(x[b, idx].astype(np.float64))[None])
            assert float((hs[b, idx] - comp[0]).abs().max()) <= 1e-12
        for t in range(T):
            if valid[b, t]:
                continue
            before = idx[idx < t]
            if len(before):
                assert torch.equal(hs[b, t], hs[b, before[-1]])
                assert float((hs[b, t] - comp[0, len(before) - 1]).abs().max()) <= 1e-12
            else:
                assert float(hs[b, t].abs().max()) == 0.0


def test_reference_row_subset():
    rng = np.random.default_rng(4)
    B, T, F, H, K = 6, 8, 5, 3, 2
    w = R.random_weights(rng, F, H, K, scale=2.0)
    x, _ = R.masked_input(rng, B, T, F)
    y, h = R.model_forward(x, w, K)
    ys, hsub = R.model_forward(x, w, K, rows=[4, 0, 5])
    assert np.array_equal(ys, y[[4, 0, 5]]) and np.array_equal(hsub, h[[4, 0, 5]])


def _params(K=3, H=13, F=20):
    return dict(mask_value=-1., maxseq=10, input_dim=F, output_dim=F, K_layers=K, hidden_dim=H)


def test_build_lstm_structure_and_initialisers():
    from drnmf_amd import layers
    K, H, F = 3, 13, 20
    m = layers.build_lstm(_params(K, H, F), device="cpu")
    kinds = [type(l).__name__ for l in m.layers]
    assert kinds == ["InputLayer", "Masking"] + ["LSTM"] * K + ["TimeDistributed", "TimeDistributed"]
    assert type(m.layers[-2].layer).__name__ == "Dense" and type(m.layers[-1].layer).__name__ == "Activation"
    assert m.layers[1].mask_value == -1.
    w = m.get_weights()
    shapes = [a.shape for a in w]
    assert shapes == [(F, 4 * H), (H, 4 * H), (4 * H,)] + [(H, 4 * H), (H, 4 * H), (4 * H,)] * (K - 1) + \
        [(H, F), (F,)]
    for k in range(K):
        l = m.lstms[k]
        assert l.weight_names == [l.name + "/kernel:0", l.name + "/recurrent_kernel:0", l.name + "/bias:0"]
        assert re.match(r"lstm_\d+$", l.name)
        b = w[3 * k + 2]
        assert np.all(b[H:2 * H] == 1) and np.all(b[:H] == 0) and np.all(b[2 * H:] == 0)   # unit_forget_bias
        U = w[3 * k + 1].astype(np.float64)
        np.testing.assert_allclose(U @ U.T, np.eye(H), atol=1e-5)                        # orthogonal
        lim = np.sqrt(6.0 / ((F if k == 0 else H) + 4 * H))
        assert np.abs(w[3 * k]).max() <= lim                                             # glorot_uniform
    assert np.all(w[-1] == 0) and np.abs(w[-2]).max() <= np.sqrt(6.0 / (H + F))
    assert m.lstms[0].recurrent_activation == "hard_sigmoid"
    m2 = layers.build_lstm(dict(_params(), recurrent_activation="sigmoid"), device="cpu")
    assert m2.lstms[0].recurrent_activation == "sigmoid"
    with pytest.raises(ValueError):
        layers.build_lstm(dict(_params(), output_dim=21), device="cpu")
    with pytest.raises(NotImplementedError):
        m.compile(loss="mse", optimizer="adam")
    new = [a + 1 for a in w]
    m.set_weights(new)
    for a, b in zip(new, m.get_weights()):
        np.testing.assert_array_equal(a, b)


def test_lstm_weight_files_round_trip(tmp_path):
    from drnmf_amd import layers, h5lite
    m = layers.build_lstm(_params(), device="cpu")
    tree = m.weights_tree()
    names = [l.name for l in m.lstms] + [m.layers[-2].name]
    assert list(tree["layer_names"]) == names
    assert list(tree[names[-1] + "/weight_names"]) == [m.dense.name + "/kernel:0", m.dense.name + "/bias:0"]
    w0 = m.get_weights()
    paths = [str(tmp_path / "w.npz")]
    if h5lite.available():
        paths.append(str(tmp_path / "w.h5"))
    for path in paths:
        m.save_weights(path)
        m2 = layers.build_lstm(_params(), device="cpu")
        m2.load_weights(path)
        for a, b in zip(w0, m2.get_weights()):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert a.tobytes() == b.tobytes()
    # a file as Keras would name it (other layer names): matched in order
    ref = {"layer_names": np.array(["lstm_91", "lstm_92", "lstm_93", "time_distributed_9"])}
    for src, dst in zip(names, ref["layer_names"]):
        wn = [str(n) for n in tree[src + "/weight_names"]]
        rn = [dst + n[n.index("/"):] for n in wn]
        ref[dst + "/weight_names"] = np.array(rn)
        for a, b in zip(wn, rn):
            ref[dst + "/" + b] = tree[src + "/" + a] * 2
    m.load_weights_tree(ref)
    for a, b in zip(w0, m.get_weights()):
        np.testing.assert_array_equal(2 * a, b)


def _declared():
    src = open(HDR).read()
    return set(re.findall(r"\b(drnmf_lstm_[a-z0-9_]+)\s*\(", src))


def test_lstm_header_is_plain_c_and_matches_the_binding(capi, tmp_path):
    declared = _declared()
    assert declared == set(capi.LSTM_SIGNATURES), declared ^ set(capi.LSTM_SIGNATURES)
    assert not (declared & set(capi.SIGNATURES))
    assert "drnmf_lstm" not in open(os.path.join(ROOT, "include", "drnmf.h")).read()
    L = capi.lib()
    for name in sorted(declared):
        assert hasattr(L, name), "libdrnmf.so does not export %s" % name
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "no C compiler"
    src = tmp_path / "lstm_header_check.c"
    src.write_text('#include "drnmf_lstm.h"\ntypedef void (*fn_t)(void);\nstatic const fn_t refs[] = {\n' +
                   "".join("    (fn_t)%s,\n" % n for n in sorted(declared)) +
                   "};\nint main(void) { return refs[0] != 0 ? 0 : 1; }\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_lstm_entry_points_validate_without_a_gpu(capi):
    """On a drnmf_create_unbound handle (no device): malformed descriptors and row strides -> DRNMF_ERR_INVALID_ARG,
    a short workspace or params buffer -> DRNMF_ERR_WORKSPACE, before anything is enqueued."""
    from drnmf_amd import ops
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)          # never dereferenced: validation fails first
        good = ops.make_lstm_desc(4, 10, 33, 13, 2)
        need = L.drnmf_lstm_workspace_bytes(ctypes.byref(good))
        pneed = L.drnmf_lstm_params_bytes(ctypes.byref(good))
        assert need > 4 * 10 * 13 * 4 * 4 and pneed > 0
        bad = []
        for field, v in (("B", 0), ("T", -1), ("F", 0), ("H", 0), ("K", 0), ("recurrent_activation", 2),
                         ("recurrent_activation", 99)):
            d = ops.make_lstm_desc(4, 10, 33, 13, 2)
            setattr(d, field, v)
            bad.append(d)
        for d in bad:
            rc = L.drnmf_lstm_forward(h, ctypes.byref(d), fake, -1.0, fake, fake, 16, fake, need, None)
            assert rc == -1, rc                      # DRNMF_ERR_INVALID_ARG
            assert L.drnmf_lstm_head_forward(h, ctypes.byref(d), fake, 16, fake, fake, None) == -1
            if d.F <= 0 or d.H <= 0 or d.K <= 0 or d.recurrent_activation not in (3, 5):
                assert L.drnmf_lstm_prepare_params(h, ctypes.byref(d), fake, fake, fake, fake, fake, fake,
                                                   fake, pneed, None) == -1
        assert L.drnmf_lstm_forward(h, None, fake, -1.0, fake, fake, 16, fake, need, None) == -1
        rc = L.drnmf_lstm_forward(h, ctypes.byref(good), fake, -1.0, fake, fake, 16, fake, need - 1, None)
        assert rc == -4, rc                          # DRNMF_ERR_WORKSPACE
        assert b"workspace" in L.drnmf_last_error(h)
        rc = L.drnmf_lstm_forward(h, ctypes.byref(good), None, -1.0, fake, fake, 16, fake, need, None)
        assert rc == -1
        rc = L.drnmf_lstm_forward(h, ctypes.byref(good), fake, -1.0, fake, fake, 12, fake, need, None)
        assert rc == -1, rc                          # row stride ld_h < H
        assert L.drnmf_lstm_head_forward(h, ctypes.byref(good), fake, 12, fake, fake, None) == -1
        rc = L.drnmf_lstm_prepare_params(h, ctypes.byref(good), fake, None, fake, fake, fake, fake, fake, pneed,
                                         None)
        assert rc == -1                              # K = 2 needs kernel_rest
        rc = L.drnmf_lstm_prepare_params(h, ctypes.byref(good), fake, fake, fake, fake, fake, fake, fake,
                                         pneed - 1, None)
        assert rc == -4, rc                          # params buffer too short
        assert L.drnmf_lstm_prepare_params(None, ctypes.byref(good), fake, fake, fake, fake, fake, fake,
                                           fake, pneed, None) == -1
        # Two faults at once: the inference and the training entries order their checks differently, and each keeps
        # its order (codes and texts as the library gave them before its host drivers were folded).
        dp = ctypes.byref(good)
        tneed = L.drnmf_lstm_train_workspace_bytes(dp)
        off = ctypes.c_void_p(0x100010)
        # fault -> (x, params, ld_h, workspace, bytes short of the full size)
        faults = {"NULL x, short workspace": (None, fake, 16, fake, 1),
                  "NULL workspace, NULL x": (None, fake, 16, None, 0),
                  "params off by 16, ld_h < H": (fake, off, 12, fake, 0),
                  "workspace and params off by 16": (fake, off, 16, off, 0)}
        expected = {"forward": (need, {
                        "NULL x, short workspace": (-1, "%s: NULL pointer argument"),
                        "NULL workspace, NULL x": (-1, "%s: NULL pointer argument"),
                        "params off by 16, ld_h < H": (-1, "%s: ld_h 12 < H 13"),
                        "workspace and params off by 16": (-1, "workspace/params must be 256-byte aligned")}),
                    "train_forward": (tneed, {
                        "NULL x, short workspace": (-4, "%%s: workspace %d < required %d" % (tneed - 1, tneed)),
                        "NULL workspace, NULL x": (-1, "%s: NULL workspace"),
                        "params off by 16, ld_h < H": (-1, "%s: ld_h 12 < H 13"),
                        "workspace and params off by 16": (-1, "workspace must be 256-byte aligned")})}
        for stem, (full, want) in expected.items():
            for suffix, state in (("", ()), ("_stateful", (fake, None, None, fake))):
                what = "lstm_" + stem + suffix
                fn = getattr(L, "drnmf_" + what)
                for name, (x, params, ld, ws, less) in faults.items():
                    code, text = want[name]
                    rc = fn(h, dp, x, -1.0, params, *state, fake, ld, ws, full - less, None)
                    assert rc == code, (what, name, rc)
                    assert L.drnmf_last_error(h).decode() == (text % what if "%s" in text else text), (what, name)
        rc = L.drnmf_lstm_loss_head_backward(h, dp, fake, fake, fake, 12, off, fake, fake, fake, fake, fake, fake,
                                             tneed, None)
        assert rc == -1 and L.drnmf_last_error(h) == b"lstm_loss_head_backward: ld_h 12 < H 13"
        rc = L.drnmf_lstm_loss_head_backward(h, dp, fake, fake, fake, 16, off, fake, fake, fake, fake, fake, off,
                                             tneed, None)
        assert rc == -1 and L.drnmf_last_error(h) == b"workspace must be 256-byte aligned"
        assert L.drnmf_lstm_head_forward(h, dp, fake, 12, off, fake, None) == -1
        assert L.drnmf_last_error(h) == b"lstm_head_forward: ld_h 12 < H 13"
    finally:
        L.drnmf_destroy(h)
