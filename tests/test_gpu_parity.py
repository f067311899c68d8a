"""Parity of the HIP path (through the C ABI) against the CPU oracle on the same seeded inputs.

Tolerances (fp32 kernels vs the fp64 oracle):
    hidden state  max|dh| / max|h| <= 1e-4
    mask          MSE <= 1e-8      (BASELINE.json bar: 1e-5)
"""
import numpy as np
import pytest
import torch

from oracle import drnmf_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("cell_form"),
              pytest.mark.parametrize("cell_form", ["auto", "factored"], indirect=True)]

H_TOL = 1e-4
MASK_MSE_TOL = 1e-8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (run with -m 'not gpu' on CPU boxes)")
    from drnmf_amd import _capi
    _capi.handle(0)        # fails loudly if libdrnmf.so is missing or the device is not gfx950
    return torch.device("cuda:0")


def _problem(B, T, F, r, K, untied=("log_D", "log_alph"), untie_alph=False, ragged=False, seed=3,
             perturb=0.05, alph=None, lam1=0.3, density=0.1):
    P = O.synth_problem(B, T, F, r, seed=seed, ragged=ragged, density=density)
    N = 2 * r
    a = np.float32(N / 4.0 if alph is None else alph)
    if untie_alph:
        a = a * np.ones((N,), np.float32)
    params = dict(W=P["W"], U1=np.eye(N, dtype=np.float32), Uk=np.zeros((N, N), np.float32),
                  alph=a, lam1=np.float32(lam1))
    alt, labels = O.build_alt(N, K, params, untied)
    rng = np.random.default_rng(seed)
    for k in list(alt):   # untied copies that really differ per layer
        if perturb and (k.startswith("log_D_") or k.startswith("log_alph_")):
            alt[k] = (alt[k] + perturb * rng.standard_normal(alt[k].shape)).astype(np.float32)
    return P, alt, labels, N


def _run_cell(dev, P, alt, labels, N, K, mask_value=-1.0, return_all_hidden=False,
              operand_f16=False):
    from drnmf_amd import ops
    X = P["X"]
    B, T, F = X.shape
    stack = lambda name: np.stack([alt[k] for k in dict.fromkeys(labels[name])], 0)
    logD, logA, logL = stack("log_D"), stack("log_alph"), stack("log_lam1")
    desc = ops.make_desc(B, T, F, N, K, n_D=logD.shape[0], n_alph=logA.shape[0],
                         alph_len=int(np.asarray(logA[0]).size), n_lam=logL.shape[0],
                         return_all_hidden=return_all_hidden, operand_f16=operand_f16)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    params = ops.prepare_params(desc, t(logD), t(logA.reshape(logA.shape[0], -1)),
                                t(logL.reshape(-1)))
    u = O.u_scalars(alt, np.float32)
    h = ops.cell_forward(t(X), mask_value, params, desc, t(P["log_h0"]), u)
    torch.cuda.synchronize()
    return h.cpu().numpy(), params, desc


def _oracle_cell(P, alt, labels, K, mask_value=-1.0, return_all_hidden=False):
    return O.cell_forward_factored(P["X"], O.maps_factored(alt, labels, K), O.u_scalars(alt),
                                   P["log_h0"], mask_value=mask_value,
                                   return_all_hidden=return_all_hidden)


def _check_h(h, ref):
    assert h.shape == ref.shape
    assert np.all(np.isfinite(h))
    err = np.max(np.abs(h - ref)) / max(np.max(np.abs(ref)), 1e-30)
    assert err <= H_TOL, "max|dh|/max|h| = %.3e" % err
    return err


def test_prepare_params_matches_oracle(dev):
    from drnmf_amd import ops
    P, alt, labels, N = _problem(2, 2, 21, 6, 3, untie_alph=True)
    _, params, desc = _run_cell(dev, P, alt, labels, N, 3)
    Dn, colnorm, ia, bias = [v.cpu().numpy() for v in ops.unpack_params(params, desc)]
    ref = O.maps_factored(alt, labels, 3)
    for k in range(3):
        np.testing.assert_allclose(Dn[k, :21, :N], ref[k][0], rtol=2e-6, atol=1e-9)
        assert np.all(Dn[k, 21:, :] == 0) and np.all(Dn[k, :, N:] == 0)
        np.testing.assert_allclose(ia[k, :N], ref[k][1], rtol=2e-6)
        np.testing.assert_allclose(bias[k, :N], ref[k][2], rtol=2e-6)
        assert np.all(bias[k, N:] < -1e29)
        np.testing.assert_allclose(np.sum(Dn[k].astype(np.float64) ** 2, 0)[:N], 1.0, rtol=1e-5)


@pytest.mark.parametrize("cfg", [
    dict(B=3, T=5, F=21, r=6, K=4),                                  # ragged dims, untied
    dict(B=16, T=4, F=64, r=32, K=3, untied=()),                     # exact tiles, tied
    dict(B=5, T=6, F=33, r=8, K=1),                                  # K=1: first == last layer
    dict(B=4, T=6, F=40, r=10, K=2, untie_alph=True),                # per-atom alpha
    dict(B=17, T=3, F=257, r=100, K=5),                              # shipped shape (C3), 2 row tiles
    dict(B=1, T=12, F=513, r=100, K=10, untied=()),                  # BASELINE config 1 shape
    dict(B=2, T=3, F=1025, r=24, K=2),                               # F > one operand group
    dict(B=3, T=4, F=21, r=6, K=3, untied=("log_D", "log_alph", "log_lam1")),
    dict(B=2, T=2, F=1025, r=4000, K=3, alph=1600.0),                # BASELINE config 5 width
    dict(B=33, T=2, F=514, r=17, K=2),                               # two tail bins, odd r, 3 row tiles
    dict(B=2, T=3, F=16, r=1, K=2),                                  # N = 2: a single atom pair
    dict(B=1, T=1, F=5, r=3, K=2),                                   # fewer bins than one tile, one frame
    dict(B=130, T=2, F=513, r=1000, K=3, alph=400.0, ragged=True),   # 9 row tiles
    dict(B=250, T=3, F=513, r=1000, K=2, alph=400.0, ragged=True),   # inference slab (enhance.py:1189): 2 row blocks per workgroup
    dict(B=250, T=2, F=512, r=1000, K=2, alph=400.0, untied=()),     # 2 row blocks, no tail bin, tied
])
def test_cell_forward_matches_oracle(dev, cfg):
    cfg = dict(cfg)
    K = cfg.pop("K")
    P, alt, labels, N = _problem(K=K, **cfg)
    h, _, _ = _run_cell(dev, P, alt, labels, N, K)
    _check_h(h, _oracle_cell(P, alt, labels, K))


def test_cell_forward_long_sequence_does_not_drift(dev):
    """The state is carried over every frame: fp32 rounding must not accumulate along a long
    utterance (T = 600 frames x K = 5 layers = 3000 dependent layer-steps; the ISTA map is
    contractive, so the error stays at the single-step level)."""
    K = 5
    P, alt, labels, N = _problem(2, 600, 65, 16, K, density=0.05)
    h, _, _ = _run_cell(dev, P, alt, labels, N, K)
    ref = _oracle_cell(P, alt, labels, K)
    scale = np.max(np.abs(ref))
    err_t = np.max(np.abs(h - ref), axis=(0, 2)) / scale
    assert err_t.max() <= H_TOL
    assert err_t[-100:].max() <= 4 * max(err_t[:100].max(), 1e-7)      # no growth with t


def test_cell_forward_masking_semantics(dev):
    """ragged lengths + a masked HEAD (outside the reference's layout contract, but defined by
    K.rnn): repeat previous output, zeros before the first valid frame, state held."""
    K = 3
    P, alt, labels, N = _problem(4, 9, 21, 6, K, ragged=True)
    P["X"][1, :2] = -1.0
    P["X"][2, :] = -1.0          # a sequence with no valid frame at all
    h, _, _ = _run_cell(dev, P, alt, labels, N, K)
    ref = _oracle_cell(P, alt, labels, K)
    _check_h(h, ref)
    assert np.all(h[1, :2] == 0) and np.all(h[2] == 0)
    L0 = int(P["lengths"][0])
    if L0 < 9:
        np.testing.assert_array_equal(h[0, L0], h[0, L0 - 1])
    # no masking requested: -1 frames are ordinary input
    h2, _, _ = _run_cell(dev, P, alt, labels, N, K, mask_value=None)
    ref2 = _oracle_cell(P, alt, labels, K, mask_value=np.nan)
    _check_h(h2, ref2)


def test_cell_forward_return_all_hidden(dev):
    K = 3
    P, alt, labels, N = _problem(3, 5, 21, 6, K, ragged=True)
    h, _, _ = _run_cell(dev, P, alt, labels, N, K, return_all_hidden=True)
    ref = _oracle_cell(P, alt, labels, K, return_all_hidden=True)
    assert h.shape == (3, 5, K * N)
    _check_h(h, ref)


def _bptt(dev, P, alt, labels, N, K, divergence="ed"):
    """Training forward (all K hiddens) and BPTT of one problem through the C ABI: [h, every gradient]."""
    from drnmf_amd import ops
    X = P["X"]
    B, T, F = X.shape
    stack = lambda name: np.stack([alt[k] for k in dict.fromkeys(labels[name])], 0)
    logD, logA, logL = stack("log_D"), stack("log_alph"), stack("log_lam1")
    desc = ops.make_desc(B, T, F, N, K, n_D=logD.shape[0], n_alph=logA.shape[0],
                         alph_len=int(np.asarray(logA[0]).size), n_lam=logL.shape[0],
                         return_all_hidden=True, divergence=divergence)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    params = ops.prepare_params(desc, t(logD), t(logA.reshape(logA.shape[0], -1)), t(logL.reshape(-1)))
    ws = ops.cell_workspace(desc, dev)
    if divergence == "ed":
        u = O.u_scalars(alt, np.float32)
        h = ops.cell_forward(t(X), -1.0, params, desc, t(P["log_h0"]), u, workspace=ws)
    else:
        u = (1.0, 0.0, 0.0)
        h = ops.cell_forward_ista(t(X), -1.0, params, desc, t(P["log_h0"]), beta=1.5, workspace=ws)
    d_out = t(np.random.default_rng(7).standard_normal((B, T, N)))
    g = ops.cell_backward(t(X), params, desc, t(P["log_h0"]), u, h, d_out, ws,
                          beta=None if divergence == "ed" else 1.5)
    torch.cuda.synchronize()
    return [h.cpu().numpy()] + [g[k].cpu().numpy() for k in sorted(g)]


def test_cell_forward_is_deterministic_and_graph_equals_plain_launches(dev, monkeypatch):
    K = 4
    P, alt, labels, N = _problem(5, 7, 65, 20, K)
    h1, _, _ = _run_cell(dev, P, alt, labels, N, K)
    h2, _, _ = _run_cell(dev, P, alt, labels, N, K)
    np.testing.assert_array_equal(h1, h2)
    # ... and the KL / beta cell, and the BPTT of the reference cell (factored or Gram form, by cell_form; the
    # Gram chains as frame graphs, not as the persistent kernels) and of the KL / beta cell: every gradient
    Pk = dict(P, X=np.where(P["X"] == -1.0, -1.0, P["X"] + 0.05).astype(np.float32))
    monkeypatch.setenv("DRNMF_PERSIST", "0")
    runs = lambda: [_bptt(dev, P, alt, labels, N, K)] + [_bptt(dev, Pk, alt, labels, N, K, dv)
                                                         for dv in ("kl", "beta")]
    graphs = runs()
    monkeypatch.setenv("DRNMF_NO_GRAPH", "1")
    for a, b in zip(graphs, runs()):
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)
    monkeypatch.delenv("DRNMF_PERSIST")
    h3, _, _ = _run_cell(dev, P, alt, labels, N, K)
    np.testing.assert_array_equal(h1, h3)


def test_kl_forward_evicts_through_the_shared_graph_cache(dev, monkeypatch):
    """More distinct KL / beta frame graphs than a handle caches (24), interleaved with a factored forward on the
    same handle: entries are evicted least recently used first, without a device synchronisation, and a call
    whose graphs were evicted (or kept) computes the same bits again."""
    monkeypatch.setenv("DRNMF_GRAM", "0")
    K = 2
    P, alt, labels, N = _problem(3, 30, 21, 6, K, density=0.3)
    P["X"] = np.where(P["X"] == -1.0, -1.0, P["X"] + 0.05).astype(np.float32)
    Pf, altf, labelsf, Nf = _problem(4, 9, 33, 8, 3)
    kl = lambda T: _run_ista_cell(dev, dict(P, X=P["X"][:, :T]), alt, labels, N, K, "kl")
    fac = lambda: _run_cell(dev, Pf, altf, labelsf, Nf, 3)[0]
    kl0, fac0 = kl(1), fac()
    for T in range(2, 31):
        kl(T)
        if T % 4 == 0:
            fac()
    np.testing.assert_array_equal(kl(1), kl0)
    np.testing.assert_array_equal(fac(), fac0)


def test_cell_reference_dense_form_agrees(dev):
    """HIP (factored) vs the reference's own op graph (dense U, materialised Gram S)."""
    K = 3
    P, alt, labels, N = _problem(2, 4, 33, 8, K)
    h, _, _ = _run_cell(dev, P, alt, labels, N, K)
    Wk, Uk, bk, Sk = O.maps_dense(alt, labels, K, N)
    _check_h(h, O.cell_forward_dense(P["X"], Wk, Uk, bk, Sk, P["log_h0"]))


def test_head_matches_oracle(dev):
    from drnmf_amd import ops
    rng = np.random.default_rng(0)
    # (>= 2048 rows take the two-GEMM form of csrc/head.hip: A through the mask buffer, ratio in the
    # second epilogue; r = 7 there = contraction not a multiple of 4, the scalar staging path)
    for rows_shape, r, F, square in [((3, 7), 6, 21, False), ((130,), 100, 257, False),
                                     ((2, 5), 7, 33, True), ((257,), 16, 513, False),
                                     ((2100,), 100, 257, False), ((16, 140), 24, 513, True),
                                     ((2050,), 7, 33, False), ((5, 500), 1000, 513, False)]:
        h = np.abs(rng.standard_normal(rows_shape + (2 * r,))).astype(np.float32) * \
            (rng.random(rows_shape + (2 * r,)) < 0.3)
        kc = (rng.standard_normal((r, F)) - 2).astype(np.float32)
        kn = (rng.standard_normal((r, F)) - 2).astype(np.float32)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        m, A, Bn = ops.head_forward(t(h), t(kc), t(kn), square=square, want_ab=True)
        torch.cuda.synchronize()
        mr, Ar, Br = O.head_forward(h, kc, kn, square=square)
        np.testing.assert_allclose(A.cpu().numpy(), Ar, rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(Bn.cpu().numpy(), Br, rtol=2e-5, atol=1e-7)
        mm = m.cpu().numpy()
        assert np.mean((mm - mr) ** 2) <= MASK_MSE_TOL
        assert np.all(mm > 0) and np.all(mm <= 1.0 + 1e-6)


@pytest.mark.parametrize("square", [False, True])
def test_model_predict_on_batch_matches_oracle(dev, square):
    from drnmf_amd import layers
    B, T, F, r, K = 6, 10, 65, 12, 4
    P = O.synth_problem(B, T, F, r, seed=11, ragged=True, density=0.1)
    N = 2 * r
    p = dict(input_dim=F, hidden_dim=N, output_dim=F, mask_value=-1., maxseq=T, K_layers=K,
             W=P["W"], alph=N / 4.0, lam1=0.3, params_untied=["log_D", "log_alph"],
             params_trainable=["log_D", "log_alph"])
    if square:
        p["transform_before_irm"] = "square"
    model = layers.build_unfolded_snmf(p)
    # weights round trip (enhance.py:1187 model_irm.set_weights(model.get_weights()))
    w = model.get_weights()
    rng = np.random.default_rng(1)
    w2 = [a + (0.03 * rng.standard_normal(a.shape)).astype(np.float32)
          if i not in (0,) and a.ndim == 2 and a.shape[0] != a.shape[1] else a
          for i, a in enumerate(w)]
    model.set_weights(w2)
    irm = model.predict_on_batch(P["X"])
    names = ["log_h0"] + list(model.cell._alt.keys()) + ["kc", "kn"]
    wd = dict(zip(names, w2))
    alt = {k: wd[k] for k in model.cell._alt.keys()}
    ref, _ = O.model_forward(P["X"], alt, model.cell.maps_from_alt.labels_per_k, K, wd["log_h0"],
                             wd["kc"], wd["kn"], mask_value=-1., square=square)
    assert irm.shape == (B, T, F)
    mse = np.mean((irm - ref) ** 2)
    assert mse <= MASK_MSE_TOL, "mask MSE %.3e" % mse
    # keras Model.predict = the slab loop of enhance.py:1189-1193 in one call (copies on their own
    # streams): the same bits as that loop, for a slab size that divides n, one that does not, one >= n
    for bs in (2, 4, 250):
        loop = np.concatenate([model.forward(torch.from_numpy(P["X"][s:s + bs]).to(dev)).cpu().numpy()
                               for s in range(0, B, bs)])
        assert np.array_equal(model.predict(P["X"], batch_size=bs), loop), bs
        assert np.array_equal(np.concatenate([model.predict_on_batch(P["X"][s:s + bs])
                                              for s in range(0, B, bs)]), loop), bs
    assert model.predict(P["X"][:0]).shape == (0, T, F)
    # layer indices enhance.py:311-315 relies on
    assert model.layers[-5 if square else -3].name == "clean_est"
    assert model.layers[-4 if square else -2].name == "noise_est"
    assert model.layers[0].name == "masking_1_input"


@pytest.mark.parametrize("r,K", [(12, 4), (100, 3)])       # (factored launches; Gram form / persistent chains)
def test_length_aware_predict_equals_the_padded_run(dev, r, K):
    """VERDICT r5 missing 3 (enhance.py:1181-1203 pads every utterance to T_max and crops afterwards): `predict`
    sorts the utterances by valid length and runs every slab at its own length.  Ragged set, lengths 0.2 .. 1.0
    of T_max, one sequence without any valid frame, one masked frame INSIDE a sequence: the full [n, T, F] array
    -- padding frames included, which repeat the last output as K.rnn's masked steps do -- equals the run at
    T_max bit for bit, with the lengths read off x and with the lengths the caller's data set knows."""
    from drnmf_amd import layers
    n, T, F = 13, 96, 65
    P = O.synth_problem(n, T, F, r, seed=19, ragged=False, density=0.1)
    N = 2 * r
    X = P["X"].copy()
    rng = np.random.default_rng(5)
    lens = rng.integers(int(0.2 * T), T + 1, size=n)
    lens[3], lens[7] = T, 0
    for i, L in enumerate(lens):
        X[i, L:] = -1.0
    X[5, 4] = -1.0                                   # a masked frame in the middle: still inside the length
    p = dict(input_dim=F, hidden_dim=N, output_dim=F, mask_value=-1., maxseq=T, K_layers=K,
             W=P["W"], alph=N / 4.0, lam1=0.3, params_untied=["log_D", "log_alph"],
             params_trainable=["log_D", "log_alph"])
    model = layers.build_unfolded_snmf(p)
    assert np.array_equal(layers.UnfoldedSNMFModel.valid_lengths(X, -1.0), lens)
    for bs in (5, 250):
        padded = model.predict(X, batch_size=bs, length_aware=False)
        loop = np.concatenate([model.forward(torch.from_numpy(X[s:s + bs]).to(dev)).cpu().numpy()
                               for s in range(0, n, bs)])
        assert np.array_equal(padded, loop)
        assert np.array_equal(model.predict(X, batch_size=bs), padded), bs
        assert np.array_equal(model.predict(X, batch_size=bs, lengths=lens), padded), bs
    # one slab through predict_on_batch: trimmed to the longest sequence in it
    sub = [0, 1, 2, 4]
    assert np.array_equal(model.predict_on_batch(X[sub]), model.predict(X[sub], batch_size=4, length_aware=False))
    with pytest.raises(ValueError):
        model.predict(X, lengths=lens[:-1])
    model.free_predict_buffers()


def test_full_size_layer_against_oracle(dev):
    """BASELINE config 2 dictionary size (F=513, N=2000, K=25, B=64) on 2 frames: every kernel
    instantiation and grid the benchmark uses, checked against the fp64 oracle."""
    K = 25
    P, alt, labels, N = _problem(64, 2, 513, 1000, K, perturb=0.0, alph=400.0, lam1=1.0,
                                 density=0.02, seed=7654)
    h, _, _ = _run_cell(dev, P, alt, labels, N, K)
    ref = _oracle_cell(P, alt, labels, K)
    _check_h(h, ref)
    # size-independent properties at full size: non-negativity and exact sparsity pattern
    assert np.all(h >= 0)
    agree = np.mean((h > 0) == (ref > 0))
    assert agree > 0.9999


def test_full_size_full_length_properties(dev):
    """BASELINE config 2 at its FULL size (F=513, N=2000, K=25 untied, B=64, T=2000: 98,000 cell
    launches replayed from hipGraphs) through size-independent properties:
      * prefix: the first 48 frames equal a 48-frame run on the same inputs, bit for bit;
      * rows: the first 16 utterances run alone give the same rows (within H_TOL: another split of
        the contraction);
      * chaining: two stateful 1000-frame halves equal the one 2000-frame run (within H_TOL);
      * a frame deep in the sequence (t = 1999) against the fp64 oracle stepped ONCE from the
        device's own state at t = 1998 (tolerance H_TOL);
      * masks of the head on the last frames are in (0, 1]."""
    from drnmf_amd import layers, ops
    B, T, F, r, K = 64, 2000, 513, 1000, 25
    N = 2 * r
    rng = np.random.Generator(np.random.PCG64(7654))
    W = rng.random((F, N)) ** 4
    W = (W / np.sqrt((W * W).sum(0, keepdims=True))).astype(np.float32)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    Wt = torch.from_numpy(W).to(dev)
    X = torch.empty((B, T, F), dtype=torch.float32, device=dev)
    for b in range(B):                      # synthetic mixture, generated on the device
        Ht = (torch.rand((T, N), generator=g, device=dev) < 0.02) * \
            torch.rand((T, N), generator=g, device=dev) * 5.0
        X[b] = Ht @ Wt.t() + 0.01 * torch.rand((T, F), generator=g, device=dev)
    p = dict(input_dim=F, hidden_dim=N, output_dim=F, mask_value=-1., maxseq=T, K_layers=K, W=W,
             alph=400.0, lam1=1.0, params_untied=["log_D", "log_alph"],
             params_trainable=["log_D", "log_alph"])
    np.random.seed(3)
    model = layers.build_unfolded_snmf(p, device=dev)
    cell = model.cell
    w = cell.get_weights()                  # untied copies that really differ per layer
    prng = np.random.default_rng(5)
    names = cell.weight_names
    for i, n in enumerate(names):
        if "log_D_" in n or "log_alph_" in n:
            w[i] = (w[i] + 0.02 * prng.standard_normal(w[i].shape)).astype(np.float32)
    cell.set_weights(w)
    h = cell.call(X, mask_value=-1.)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(h).all()) and float(h.min()) >= 0.0
    # prefix and row independence
    assert torch.equal(cell.call(X[:, :48].contiguous(), mask_value=-1.), h[:, :48])
    # (16 rows alone use more atom ranges per bin tile -- another summation order: H_TOL, not bits)
    h16 = cell.call(X[:16].contiguous(), mask_value=-1.)
    assert float((h16 - h[:16]).abs().max()) <= H_TOL * float(h[:16].max())
    # stateful chaining of two halves (state enters as given: start both from the same h0)
    alt = {n[len(cell.name) + 1:]: v for n, v in zip(names[1:], w[1:])}
    labels = cell.maps_from_alt.labels_per_k
    desc = cell.prepare(B, T // 2)
    h0 = torch.from_numpy(np.tile(O.softplus(w[0].astype(np.float64)).astype(np.float32), (B, 1))).to(dev)
    st = torch.empty((B, N), dtype=torch.float32, device=dev)
    ha = ops.cell_forward(X[:, :T // 2].contiguous(), -1., cell._params_block, desc, cell.log_h0,
                          cell._u, initial_state=h0, final_state=st)
    hb = ops.cell_forward(X[:, T // 2:].contiguous(), -1., cell._params_block, desc, cell.log_h0,
                          cell._u, initial_state=st, final_state=st)
    # (a supplied state enters with its row sum added in another order than the per-atom-block
    # partial sums the kernels chain between frames: H_TOL, not bits)
    tol = H_TOL * float(h.max())
    assert float((ha - h[:, :T // 2]).abs().max()) <= tol
    assert float((hb - h[:, T // 2:]).abs().max()) <= tol
    # one oracle step deep in the sequence, from the device's own state
    rows = slice(0, 8)
    ref = O.cell_forward_factored(X[rows, T - 1:].cpu().numpy(), O.maps_factored(alt, labels, K),
                                  O.u_scalars(alt), w[0], mask_value=-1.0,
                                  initial_state=h[rows, T - 2].cpu().numpy().astype(np.float64))
    _check_h(h[rows, T - 1:].cpu().numpy(), ref)
    mask = ops.head_forward(h[:, T - 4:].contiguous(), model.clean.kernel, model.noise.kernel)
    assert float(mask.min()) > 0.0 and float(mask.max()) <= 1.0 + 1e-6


# ------------------------------------------------------------------ frame-parallel ISTA / MU
@pytest.mark.parametrize("tag", ["a", "b", "c"])
@pytest.mark.parametrize("name", ["ed", "kl", "beta"])
def test_ista_matches_reference_golden_vectors(dev, golden, tag, name):
    """HIP frame-parallel ISTA vs the outputs of the reference's own ista_* (golden fixtures)."""
    from drnmf_amd import ops
    g = golden
    W, x, H0 = g["ista_%s_W" % tag], g["ista_%s_x" % tag], g["ista_%s_H0" % tag]
    lam1, K = float(g["ista_%s_lam1" % tag]), int(g["ista_%s_K" % tag])
    alph = float(g["ista_%s_alph" % tag] if name == "ed" else g["ista_%s_alph_kl" % tag])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    H = t(H0.T)                                   # row layout: frames are rows
    ops.ista_forward(t(x.T), t(W), H, lam1, alph, K, divergence=name,
                     beta=float(g["ista_beta_value"]))
    torch.cuda.synchronize()
    ref = g["ista_%s_%s_H" % (tag, name)].T.astype(np.float64)
    got = H.cpu().numpy()
    err = np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-30)
    assert err <= 2e-5, "ista_%s %s: rel err %.3e" % (name, tag, err)


def test_ista_large_ragged_shape_vs_oracle(dev):
    """several 128x128 GEMM tiles with ragged edges (n=300, F=257, N=200)."""
    from drnmf_amd import ops
    rng = np.random.default_rng(5)
    n, F, N, K = 300, 257, 200, 7
    W = rng.random((F, N)) ** 4
    W = (W / np.sqrt((W * W).sum(0, keepdims=True))).astype(np.float32)
    Ht = ((rng.random((N, n)) < 0.05) * rng.random((N, n)) * 3).astype(np.float32)
    x = (W @ Ht + 0.01 * rng.random((F, n))).astype(np.float32)
    H0 = (0.1 * rng.random((N, n))).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    H = t(H0.T)
    ops.ista_forward(t(x.T), t(W), H, 0.5, 50.0, K)
    torch.cuda.synchronize()
    ref = O.ista_ed(x.astype(np.float64), W.astype(np.float64), H0.astype(np.float64), 0.5, 50.0, K)
    err = np.max(np.abs(H.cpu().numpy() - ref.T)) / np.max(np.abs(ref))
    assert err <= 2e-5, err


@pytest.mark.parametrize("F", [64, 34, 48, 130, 129, 257])
@pytest.mark.parametrize("name", ["ed", "kl", "beta"])
def test_ista_bin_counts_around_the_tile_size(dev, F, name):
    """The X^ / G GEMMs run on whole 16-bin tiles and the 1-2 odd bins of a 2^k+1 STFT go through
    a separate rank-1 path: F = 64, 48 (no odd bins), 34, 130 (two), with the goldens covering one;
    F = 129, 257: the one odd bin behind whole 128-column tiles rides on the X^ product (gemm_nt.h THIN)."""
    from drnmf_amd import ops
    rng = np.random.default_rng(F)
    N, n, K = 24, 37, 6
    W = rng.random((F, N)) ** 2
    W = (W / np.sqrt((W * W).sum(0, keepdims=True))).astype(np.float32)
    x = (W @ ((rng.random((N, n)) < 0.3) * rng.random((N, n))) + 0.05).astype(np.float32)
    H0 = (0.1 + 0.1 * rng.random((N, n))).astype(np.float32)
    alph = 40.0 * N if name != "ed" else 4.0
    fn = dict(ed=O.ista_ed, kl=O.ista_kl, beta=lambda *a, **k: O.ista_beta(*a, beta=1.5, **k))[name]
    want = fn(x.astype(np.float64), W.astype(np.float64), H0.astype(np.float64), 0.1, alph, K)
    want = want[0] if isinstance(want, tuple) else want
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    H = t(H0.T)
    ops.ista_forward(t(x.T), t(W), H, 0.1, alph, K, divergence=name, beta=1.5)
    torch.cuda.synchronize()
    got = H.cpu().numpy().T
    assert np.max(np.abs(got - want)) <= 2e-5 * max(np.max(np.abs(want)), 1e-6)


@pytest.mark.parametrize("beta,F", [(2.0, 65), (1.0, 65), (1.5, 65), (0.0, 65), (0.5, 65), (3.0, 65),
                                    (2.0, 129), (2.0, 257), (1.0, 129)])
def test_mu_inference_and_irm_vs_oracle(dev, beta, F):
    """F = 129, 257: one bin behind whole 128-column tiles -- the odd output column of W H rides on the full
    tiles' staging (csrc/gemm_nt.h THIN; one and two column tiles)."""
    from drnmf_amd import ops
    rng = np.random.default_rng(6)
    n, N, iters = 150, 24, 30
    W = rng.random((F, N)).astype(np.float32) * 3            # deliberately NOT normalised
    V = (W @ ((rng.random((N, n)) < 0.3) * rng.random((N, n))) + 1e-3).astype(np.float32)
    if beta != 2.0:
        V[rng.random(V.shape) < 0.02] = 0.0                  # zeros get floored for beta != 2
    H0 = rng.random((N, n)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    H = t(H0.T)
    H, Wn, irm = ops.mu_forward(t(V.T), t(W), H, 0.1, iters, beta=beta, want_irm=True)
    torch.cuda.synchronize()
    Hr, Wr = O.mu_infer(V.astype(np.float64), W.astype(np.float64), H0.astype(np.float64), 0.1,
                        iters, beta=beta)
    np.testing.assert_allclose(Wn.cpu().numpy(), Wr, rtol=1e-5)
    err = np.max(np.abs(H.cpu().numpy() - Hr.T)) / np.max(np.abs(Hr))
    assert err <= 2e-4, "beta=%g rel err %.3e" % (beta, err)
    irm_r = O.snmf_irm(Wr, Hr, N // 2)
    assert np.mean((irm.cpu().numpy() - irm_r.T) ** 2) <= MASK_MSE_TOL


# ------------------------------------------------------------------ STFT-magnitude front end
@pytest.mark.parametrize("N,hop,nsampl,int16", [(64, 16, 1000, False), (512, 128, 16000, True),
                                                (128, 32, 3000, False), (2048, 512, 9999, True),
                                                (4096, 2048, 20000, False),
                                                (1024, 512, 40000, True), (1024, 256, 777, False),
                                                (4096, 1024, 20000, True)])
def test_stft_mag_vs_oracle(dev, N, hop, nsampl, int16):
    from drnmf_amd import ops
    rng = np.random.default_rng(N + hop)
    n_sig = 3
    if int16:
        pcm = rng.integers(-20000, 20000, size=(n_sig, nsampl)).astype(np.int16)
        xf = O.wav_int16_to_float(pcm)
        tp = torch.from_numpy(pcm).to(dev)
    else:
        xf = rng.standard_normal((n_sig, nsampl)).astype(np.float32)
        tp = torch.from_numpy(xf).to(dev)
    mag = ops.stft_mag(tp, N=N, hop=hop)
    torch.cuda.synchronize()
    w = O.sqrt_hann(N)
    nf = O.stft_frames(nsampl, N, hop)
    assert tuple(mag.shape) == (n_sig, nf, N // 2 + 1)
    got = mag.cpu().numpy()
    for s in range(n_sig):
        ref = O.stft_mag(xf[s], N, hop, w).T          # (frames, bins)
        err = np.max(np.abs(got[s] - ref)) / np.max(np.abs(ref))
        assert err <= 2e-5, "N=%d rel err %.3e" % (N, err)
    assert np.all(got[:, 0, :] == 0)                   # the all-zero leading frame


# ------------------------------------------------------------------ sparse-NMF dictionary training
@pytest.mark.parametrize("beta,cf,F", [(2.0, "ed", 65), (1.0, "kl", 65), (1.5, None, 65), (0.0, "is", 65),
                                       (0.5, None, 65), (3.0, None, 65),
                                       (2.0, "ed", 129), (1.0, "kl", 129), (1.5, None, 129),
                                       (2.0, "ed", 257), (1.0, "kl", 257)])
def test_snmf_training_matches_oracle(dev, beta, cf, F):
    """W/H multiplicative updates + renormalisation + objective vs the numpy restatement of
    sparse_nmf_gpu.m (same explicit inits), incl. a frozen half of the dictionary.  F = 129 / 257: the
    513-bin shape in small -- the odd bin as the rider column of the lambda products (with the objective
    summed in the same epilogue) and as the streamed odd row of the W statistics."""
    from drnmf_amd import ops
    rng = np.random.default_rng(8)
    r, n, iters = 12, 300, 25
    Wt = rng.random((F, r))
    V = (Wt @ (rng.random((r, n)) * (rng.random((r, n)) < 0.4)) + 1e-3).astype(np.float32)
    if beta != 2.0:
        V[rng.random(V.shape) < 0.01] = 0.0
    W0 = rng.random((F, r)).astype(np.float32) * 2
    H0 = rng.random((r, n)).astype(np.float32)
    w_ind = np.array([False] * 5 + [True] * 7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    tr = ops.SnmfTrainer(t(V.T), t(W0), t(H0.T), beta=beta)
    mask = torch.from_numpy(w_ind.astype(np.uint8)).to(dev)
    objs = [tr.step(0.1, mask, True).cpu().numpy() for _ in range(iters)]
    Wr, Hr, oref = O.sparse_nmf_train(V.astype(np.float64), W0.astype(np.float64),
                                      H0.astype(np.float64), 0.1, iters, 0.0, beta, w_ind)
    W, H = tr.W.cpu().numpy(), tr.H.cpu().numpy().T
    assert np.max(np.abs(W - Wr)) / np.max(np.abs(Wr)) <= 5e-4
    assert np.max(np.abs(H - Hr)) / np.max(np.abs(Hr)) <= 5e-4
    np.testing.assert_allclose(np.array(objs)[:, 1], oref["cost"], rtol=2e-4)
    np.testing.assert_allclose(np.array(objs)[:, 0], oref["div"], rtol=2e-4)
    np.testing.assert_allclose((W * W).sum(0), 1.0, rtol=1e-5)
    # frozen columns only get renormalised (they were unit-norm after init): unchanged direction
    W0n = W0 / np.sqrt((W0 * W0).sum(0))
    np.testing.assert_allclose(W[:, :5], W0n[:, :5], rtol=1e-5)
    assert np.all(np.diff(np.array(objs)[:, 1]) <= 1e-4 * np.array(objs)[:-1, 1])


def test_sparse_nmf_host_api_chunks_and_two_stage(dev):
    """sparse_nmf / train_snmf mirror snmf.sparse_nmf_matlab / enhance.train_snmf: chunking,
    convergence stop, two-stage training with the speech half frozen."""
    from drnmf_amd import snmf
    rng = np.random.default_rng(9)
    F, r, n = 33, 6, 500
    clean = (rng.random((F, r)) @ (rng.random((r, n)) * (rng.random((r, n)) < 0.3)) + 1e-3).astype(np.float32)
    noise = (rng.random((F, r)) @ (rng.random((r, n)) * (rng.random((r, n)) < 0.3))).astype(np.float32)
    noisy = clean + noise
    params = dict(r=r, cf="ed", sparsity=0.1, max_iter=40, conv_eps=1e-4, random_seed=2016)
    W, H, obj = snmf.sparse_nmf(clean, params)
    assert W.shape == (F, r) and H.shape == (r, n)
    assert len(obj["cost"]) <= 40 and np.all(np.diff(obj["cost"]) <= 1e-4 * obj["cost"][:-1])
    # chunked run (3 chunks): objective bookkeeping of snmf.py:66-83
    W3, H3, obj3 = snmf.sparse_nmf(clean, params, max_frame_batch_size=6)   # 6*200/6 = 200 frames
    assert len(obj3["obj_snmf_per_chunk"]) == 3 and len(obj3["cost"]) == 2 and H3.shape == (r, n)
    Wn, Hn, objn = snmf.train_snmf(clean, noisy, dict(params, max_iter=15, conv_eps=0.0))
    assert Wn.shape == (F, 2 * r) and Hn.shape == (2 * r, n)
    Wc, _, _ = snmf.sparse_nmf(clean, dict(params, max_iter=15, conv_eps=0.0))
    np.testing.assert_allclose(Wn[:, :r], Wc, rtol=1e-4, atol=1e-6)      # speech half frozen
    np.testing.assert_allclose((Wn * Wn).sum(0), 1.0, rtol=1e-5)


# ------------------------------------------------------------------ STFT -> mask -> iSTFT -> SNR
@pytest.mark.parametrize("N,hop,nsampl", [(512, 128, 16000), (1024, 256, 9999), (64, 16, 700)])
def test_stft_istft_reconstruction_and_snr(dev, N, hop, nsampl):
    from drnmf_amd import ops
    rng = np.random.default_rng(N)
    n_sig = 2
    x = (0.3 * rng.standard_normal((n_sig, nsampl))).astype(np.float32)
    tx = torch.from_numpy(x).to(dev)
    re, im, mag = ops.stft(tx, N=N, hop=hop, want_mag=True)
    w = O.sqrt_hann(N)
    nf = O.stft_frames(nsampl, N, hop)
    for s in range(n_sig):
        S = O.stft_mc(x[s], N, hop, w)                      # conjugated convention
        scale = np.max(np.abs(S))
        assert np.max(np.abs(re[s].cpu().numpy().T - S.real)) <= 2e-5 * scale
        assert np.max(np.abs(im[s].cpu().numpy().T - S.imag)) <= 2e-5 * scale
    # unmasked round trip: sqrt-Hann analysis + synthesis, hop = N/4 -> perfect reconstruction
    y = ops.istft_masked(re, im, None, nsampl, N, hop)
    torch.cuda.synchronize()
    err = np.max(np.abs(y.cpu().numpy() - x)) / np.max(np.abs(x))
    assert err <= 1e-4, err
    # masked reconstruction vs the oracle's reconstruct_x/istft_mc
    mask = rng.random((n_sig, nf, N // 2 + 1)).astype(np.float32)
    ym = ops.istft_masked(re, im, torch.from_numpy(mask).to(dev), nsampl, N, hop).cpu().numpy()
    for s in range(n_sig):
        S = O.stft_mc(x[s], N, hop, w)
        ref = O.reconstruct(S.real, S.imag, mask[s].T.astype(np.float64), hop, w, nsampl)
        assert np.max(np.abs(ym[s] - ref)) <= 1e-4 * np.max(np.abs(ref))
    snr = ops.snr_db(torch.from_numpy(ym).to(dev), tx).cpu().numpy()
    for s in range(n_sig):
        np.testing.assert_allclose(snr[s], O.snr_db(ym[s].astype(np.float64), x[s].astype(np.float64)),
                                   rtol=1e-4)
    q = ops.to_int16_wav(y[0])
    assert q.dtype == torch.int16 and int(q.abs().max()) <= 32767


def test_reconstruction_kernels_match_reference_golden(dev, golden):
    """The iSTFT and wav-quantisation kernels against the REFERENCE ITSELF: util.istft_mc(flag_noDiv=1) as
    audio_dataset.reconstruct_x calls it and util.wavwrite's int16 conversion, executed as written
    (tests/golden/make_golden.py)."""
    from drnmf_amd import ops
    g = golden
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    re, im = t(g["istft_S_re"].T[None]), t(g["istft_S_im"].T[None])          # [n_sig, n_frames, F]
    hop = int(g["istft_hop"])
    N = 2 * (re.shape[-1] - 1)
    full = g["istft_mc_x"][0]
    y = ops.istft_masked(re, im, None, full.shape[0], N, hop).cpu().numpy()[0]
    assert np.max(np.abs(y - full)) <= 1e-4 * np.max(np.abs(full))
    want = g["istft_mc_x_nsampl100"][0]
    ym = ops.istft_masked(re, im, t(g["istft_mask"].T[None]), 100, N, hop).cpu().numpy()[0]
    assert np.max(np.abs(ym - want)) <= 1e-4 * np.max(np.abs(want))
    for tag in ("quiet", "loud"):
        q = ops.to_int16_wav(t(g["wav_%s_float" % tag][0])).cpu().numpy()
        # (x / max|x| * 32767 in float32 on the device, float64 in numpy: a value on an integer boundary may
        # truncate to the neighbour)
        assert np.max(np.abs(q.astype(int) - g["wav_%s_int16" % tag].astype(int))) <= 1
        assert np.mean(q == g["wav_%s_int16" % tag]) > 0.99


def test_stateful_cell_carries_state_across_batches(dev):
    """stateful=True (custom_layers.py:296-318): two consecutive half-length calls equal one
    full-length run started from the zero state; reset_states() zeroes it again."""
    from drnmf_amd import layers
    K = 3
    P, alt, labels, N = _problem(3, 8, 21, 6, K, ragged=False)
    params = dict(W=P["W"], U1=np.eye(N, dtype=np.float32), Uk=np.zeros((N, N), np.float32),
                  alph=np.float32(N / 4.0), lam1=np.float32(0.3))
    alt_l, maps = layers.build_alt(N, K, params, params_untied=["log_D", "log_alph"])
    for k in alt_l:
        alt_l[k] = alt[k]
    cell = layers.SimpleDeepRNN(N, activation="relu", K_layers=K, alt_params=alt_l,
                                maps_from_alt=maps, flag_connect_input_to_layers=True,
                                flag_nonnegative=True, return_sequences=True, stateful=True)
    cell.build((3, 4, 21))
    cell.log_h0.copy_(torch.from_numpy(P["log_h0"]))
    x = torch.from_numpy(P["X"]).to(dev)
    h1 = cell(x[:, :4].contiguous()).cpu().numpy()
    h2 = cell(x[:, 4:].contiguous()).cpu().numpy()
    lay, u = O.maps_factored(alt, labels, K), O.u_scalars(alt)
    ref, st = O.cell_forward_factored(P["X"], lay, u, P["log_h0"], mask_value=np.nan,
                                      initial_state=np.zeros((3, N)), return_state=True)
    _check_h(np.concatenate([h1, h2], 1), ref)
    np.testing.assert_allclose(cell.states[0].cpu().numpy(), st, atol=1e-4 * np.max(np.abs(st)))
    cell.reset_states()
    assert float(cell.states[0].abs().max()) == 0.0
    h1b = cell(x[:, :4].contiguous()).cpu().numpy()
    np.testing.assert_array_equal(h1, h1b)


@pytest.mark.parametrize("nsampl,flen", [(3000, 64), (16000, 512), (777, 512)])
def test_sdr_vs_oracle(dev, nsampl, flen):
    """SDR of bss_eval_sources with one source (score_audio.m:206; BSS Eval 3.0 absent from the
    reference tree -> pinned to the published definition, oracle.sdr_db)."""
    from drnmf_amd import ops
    rng = np.random.default_rng(nsampl)
    n_sig = 3
    # speech-like coloured references (AR(2)), estimates = filtered reference + noise
    ref = np.zeros((n_sig, nsampl), np.float32)
    est = np.zeros((n_sig, nsampl), np.float32)
    for s in range(n_sig):
        w = rng.standard_normal(nsampl)
        x = np.zeros(nsampl)
        for i in range(nsampl):
            x[i] = w[i] + (1.3 * x[i - 1] if i > 0 else 0.0) - (0.6 * x[i - 2] if i > 1 else 0.0)
        ref[s] = (0.1 * x).astype(np.float32)
        est[s] = (np.convolve(ref[s], [0.8, 0.1, -0.05])[:nsampl] +
                  0.02 * (s + 1) * rng.standard_normal(nsampl)).astype(np.float32)
    ref[2, nsampl - 100:] = 0.0          # a zero-padded (shorter) signal in the batch
    est[2, nsampl - 100:] = 0.0
    out, coef, en = ops.sdr_db(torch.from_numpy(est).to(dev), torch.from_numpy(ref).to(dev),
                               flen=flen, return_parts=True)
    torch.cuda.synchronize()
    out, en = out.cpu().numpy(), en.cpu().numpy()
    for s in range(n_sig):
        want, C, num, den = O.sdr_db(est[s], ref[s], flen, return_parts=True)
        assert abs(out[s] - want) <= 1e-3, (s, out[s], want)          # dB
        np.testing.assert_allclose(en[s], [num, den], rtol=1e-6)
    # correlations alone (no solve): exact to fp64 rounding of different summation orders
    want2 = O.sdr_db(est[2, :nsampl - 100], ref[2, :nsampl - 100], flen)
    assert abs(out[2] - want2) <= 1e-3                                # padding changes nothing


def test_c_abi_status_codes_and_messages(dev):
    """Error behaviour of the boundary: every export returns a status, never
    throws or aborts, and drnmf_last_error carries the reason.  Empty inputs (B or T = 0) are
    invalid arguments, as Keras rejects an empty batch."""
    import ctypes as C
    from drnmf_amd import _capi, ops
    L = _capi.lib()
    h = _capi.handle(0)
    P, alt, labels, N = _problem(2, 3, 21, 6, 2)
    _, params, desc = _run_cell(dev, P, alt, labels, N, 2)
    x = torch.from_numpy(P["X"]).to(dev)
    out = torch.empty((2, 3, N), dtype=torch.float32, device=dev)
    ws = ops.cell_workspace(desc, dev)
    lh0 = torch.zeros(N, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd(d, xx=x, pp=params, oo=out, w=ws, wbytes=None):
        return L.drnmf_cell_forward(h, C.byref(d), _capi.ptr(xx), -1.0, _capi.ptr(pp),
                                    _capi.ptr(lh0), 1.0, 0.0, 0.0, _capi.ptr(oo), _capi.ptr(w),
                                    w.numel() if wbytes is None else wbytes, st)
    assert fwd(desc) == 0
    for field, val in (("B", 0), ("T", 0), ("K", 0), ("n_D", 3), ("alph_len", 5)):
        bad = ops.make_desc(2, 3, 21, N, 2, n_D=2, n_alph=2)
        setattr(bad, field, val)
        assert fwd(bad) == -1, field
        assert len(L.drnmf_last_error(h)) > 0
    assert fwd(desc, xx=None) == -1                                   # NULL pointer
    assert fwd(desc, wbytes=1024) == -4                               # workspace too small
    assert b"workspace" in L.drnmf_last_error(h)
    big = torch.empty(ws.numel() + 256, dtype=torch.uint8, device=dev)
    assert fwd(desc, w=big[4:], wbytes=ws.numel()) == -1              # misaligned workspace
    assert L.drnmf_cell_workspace_bytes(None) == 0
    assert L.drnmf_cell_forward(None, C.byref(desc), None, 0.0, None, None, 0.0, 0.0, 0.0, None,
                                None, 0, None) == -1                  # NULL handle
    # the Python layer turns the codes into exceptions
    with pytest.raises(ValueError):
        ops.cell_forward(x[:, :0], -1.0, params, ops.make_desc(2, 0, 21, N, 2, n_D=2, n_alph=2),
                         lh0, (1.0, 0.0, 0.0))
    Wd, H0 = torch.rand((21, N), device=dev), torch.rand((3, N), device=dev)
    with pytest.raises(ValueError):
        ops.ista_forward(x[0].abs(), Wd, H0.clone(), 0.1, 0.0, 2)     # alph must be > 0
    Hk = ops.ista_forward(x[0].abs(), Wd, H0.clone(), 0.1, 1.0, 0)    # K = 0: `for k in range(0)`
    assert torch.equal(Hk, H0)
    with pytest.raises(ValueError):
        ops.stft_mag(torch.zeros((1, 100), device=dev), N=100, hop=25)   # N not a power of two
    torch.cuda.synchronize()
    assert fwd(desc) == 0                                             # the handle is still usable


@pytest.mark.parametrize("cfg", [
    dict(B=3, T=5, F=21, r=6, K=4),
    dict(B=17, T=4, F=257, r=100, K=5, ragged=True),                 # one tail bin
    dict(B=5, T=3, F=64, r=16, K=3, untied=()),                      # whole tiles only, tied
    dict(B=2, T=2, F=1025, r=4000, K=3, alph=1600.0),                # BASELINE config 5 width
    dict(B=250, T=2, F=513, r=1000, K=2, alph=400.0),                # row-blocked kernels
    dict(B=20, T=6, F=49, r=24, K=4, ragged=True),    # odd count of 16-bin MFMA tiles + one odd bin:
                                                      # the last 32-bin chunk straddles the tail tile
    dict(B=4, T=3, F=34, r=40, K=3),                  # two odd bins
    dict(B=16, T=2, F=1025, r=4000, K=50, alph=1600.0),              # BASELINE config 5 at its depth
    dict(B=3, T=4, F=21, r=6, K=1),                   # a single layer: first and last at once (no cell_b, no prefetch)
    dict(B=70, T=3, F=65, r=150, K=3, ragged=True),   # 10 atom blocks, 3 row groups: the spare waves' shares wrap
])
def test_cell_forward_fp16_operands(dev, cfg):
    """BASELINE config 5: fp16 MFMA operands, fp32 accumulate.  Against the oracle's emulation of
    the same rounding points (tight), and against the exact fp64 oracle through the mask (the
    north-star bar: mask MSE < 1e-5; SURVEY.md 8c expects <= 1e-6 for fp16 operands)."""
    cfg = dict(cfg)
    K = cfg.pop("K")
    P, alt, labels, N = _problem(K=K, **cfg)
    h, _, _ = _run_cell(dev, P, alt, labels, N, K, operand_f16=True)
    lay, u = O.maps_factored(alt, labels, K), O.u_scalars(alt)
    emu = O.cell_forward_factored(P["X"], lay, u, P["log_h0"], operand_dtype=np.float16)
    exact = O.cell_forward_factored(P["X"], lay, u, P["log_h0"])
    assert np.all(np.isfinite(h))
    scale = max(np.max(np.abs(emu)), 1e-30)
    # fp32 accumulation order + activations that sit on an fp16 rounding boundary
    assert np.max(np.abs(h - emu)) / scale <= 2e-3
    assert np.sqrt(np.mean((h - emu) ** 2)) / scale <= 1e-4
    r = N // 2
    kc = np.log(1e-7 + P["W"][:, :r]).T
    kn = np.log(1e-7 + P["W"][:, r:]).T
    m16 = O.head_forward(h, kc, kn)[0]
    m64 = O.head_forward(exact, kc, kn)[0]
    valid = (P["X"] != -1.0).any(-1)
    assert np.mean((m16 - m64)[valid] ** 2) <= 1e-6
    # every hidden layer (what the mixed-precision BPTT consumes): same kernels, same last layer
    if cfg["B"] * cfg["r"] <= 20000:
        hall, _, _ = _run_cell(dev, P, alt, labels, N, K, return_all_hidden=True, operand_f16=True)
        # (another template instance of the same kernels: a last-bit fp32 difference ahead of an
        # fp16 rounding point can move a value by an fp16 ulp)
        assert np.max(np.abs(hall[..., (K - 1) * N:] - h)) / scale <= 2e-3
        emu_all = O.cell_forward_factored(P["X"], lay, u, P["log_h0"], operand_dtype=np.float16,
                                          return_all_hidden=True)
        assert np.max(np.abs(hall - emu_all)) / scale <= 2e-3


@pytest.mark.parametrize("square", [False, True])
def test_mask_head_matches_reference_golden(dev, golden, square):
    """The head kernels against the REFERENCE ITSELF (DenseNonNegW.call, DivideAbyAplusB._merge_function run as
    written, tests/golden/make_golden.py): through the C ABI and through the Keras-surface layers."""
    from drnmf_amd import layers, ops
    g = golden
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    h, kc, kn = t(g["head_h"]), t(g["head_kc"]), t(g["head_kn"])
    want = g["head_mask_square" if square else "head_mask"]
    m, A, Bn = ops.head_forward(h, kc, kn, square=square, want_ab=True)
    np.testing.assert_allclose(m.cpu().numpy(), want, rtol=2e-5, atol=1e-6)
    if not square:
        np.testing.assert_allclose(A.cpu().numpy(), g["head_A"], rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(Bn.cpu().numpy(), g["head_B"], rtol=2e-5, atol=1e-6)
        r, F = g["head_kc"].shape
        dn = layers.DenseNonNegW(F, use_bias=False, weights=[g["head_kc"]], device=dev)
        np.testing.assert_allclose(dn(h[..., :r].contiguous()).cpu().numpy(), g["head_A"], rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(layers.divide_A_by_AplusB([A, Bn]).cpu().numpy(), want, rtol=2e-5, atol=1e-6)


def test_fused_cell_matches_reference_step_golden(dev, golden):
    """The fused factored kernels against the REFERENCE ITSELF: build_alt's maps (enhance.py:139-206) and
    SimpleDeepRNN.step / get_initial_state (custom_layers.py:336-375) executed as written over a 5-frame
    sequence (tests/golden/make_golden.py, case seq_fused: untied log_D / log_alph at 'trained' values, U as
    initialised) -- through the C ABI directly and through the Keras-surface layer, which must pick the
    fused path by itself."""
    from drnmf_amd import layers
    g, pre = golden, "step_seq_fused_"
    alt = {k[len(pre + "alt_"):]: g[k] for k in g.files if k.startswith(pre + "alt_")}
    X, ref = g[pre + "x"], g[pre + "h"]
    B, T, F = X.shape
    N, K = ref.shape[-1], sum(1 for k in g.files if k.startswith(pre + "U_"))
    labels = {n: (["%s_%d" % (n, k) for k in range(K)] if n + "_0" in alt else [n] * K)
              for n in ("log_D", "log_alph", "log_lam1")}
    h, _, _ = _run_cell(dev, dict(X=X, log_h0=g[pre + "log_h0"]), alt, labels, N, K)
    _check_h(h, ref)
    W = g["alt_untied_da_W"]
    params = dict(W=W, U1=np.eye(N, dtype=np.float32), Uk=np.zeros((N, N), np.float32),
                  alph=g["alt_untied_da_alph"], lam1=g["alt_untied_da_lam1"])
    alt0, maps = layers.build_alt(N, K, params, ["log_D", "log_alph"])
    cell = layers.SimpleDeepRNN(N, activation="relu", K_layers=K, alt_params=alt0, maps_from_alt=maps,
                                keys_trainable=["log_D_0"], flag_connect_input_to_layers=True,
                                flag_nonnegative=True, return_sequences=True, device=dev)
    cell.build((B, T, F))
    names = [n[len(cell.name) + 1:] for n in cell.weight_names]
    cell.set_weights([g[pre + "log_h0"] if n == "log_h0" else alt[n] for n in names])
    assert not cell._dense_now
    _check_h(cell.call(torch.from_numpy(X).to(dev), mask_value=-1.).cpu().numpy(), ref)


def test_end_to_end_enhancement_pipeline(dev):
    """enhance.py's inference flow end to end on the device -- wav -> STFT stacks ->
    reshape_and_pad_stacks -> predict_on_batch in slabs -> crop -> masked iSTFT -> SNR / SDR
    (enhance.py:1185-1203, audio_dataset.py:267-278, score_audio.m:206-209) -- against the same flow
    through the oracle."""
    from drnmf_amd import data as D, layers, ops
    rng = np.random.default_rng(12)
    N_fft, hop, maxlen = 64, 16, 20
    F = N_fft // 2 + 1
    lens = [700, 433, 900]
    clean = [(0.3 * np.sin(0.05 * (i + 1) * np.arange(n)) * rng.random(n)).astype(np.float32)
             for i, n in enumerate(lens)]
    noisy = [c + 0.1 * rng.standard_normal(c.shape[0]).astype(np.float32) for c in clean]
    pcm = [np.clip(np.round(v * 32768.0), -32768, 32767).astype(np.int16) for v in noisy]
    win = O.sqrt_hann(N_fft)

    # ---- device: STFT of every utterance, concatenated [re; im] stack + frame index table ----
    re_d, im_d, nfr = [], [], []
    for p in pcm:
        re, im = ops.stft(torch.from_numpy(p).to(dev), N=N_fft, hop=hop)
        re_d.append(re[0]); im_d.append(im[0]); nfr.append(re.shape[1])
    fidx = np.stack([np.cumsum([0] + nfr[:-1]), np.cumsum(nfr)], 1)
    stack = np.concatenate([torch.cat(re_d).cpu().numpy().T, torch.cat(im_d).cpu().numpy().T], 0)
    mag = D.get_transform("mag")
    x, _, m = D.reshape_and_pad_stacks(stack, stack, fidx, transform_x=mag, transform_y=mag,
                                       pad_value=D.get_mask_value({"transform_x": "mag"}),
                                       maxlen=maxlen)
    r, K = 8, 3
    P = O.synth_problem(1, 1, F, r, seed=4)
    params = dict(input_dim=F, hidden_dim=2 * r, output_dim=F, mask_value=-1., maxseq=maxlen,
                  K_layers=K, W=P["W"], alph=4.0, lam1=0.1, params_untied=["log_D", "log_alph"],
                  params_trainable=["log_D", "log_alph"])
    model = layers.build_unfolded_snmf(params, device=dev)
    irm = np.concatenate([model.predict_on_batch(x[s:s + 2]) for s in range(0, x.shape[0], 2)])
    irm_stack = D.sequences_to_stack(irm, fidx, maxlen=maxlen)               # (F, total frames)
    snr_d, sdr_d, wav_d = [], [], []
    for u, n in enumerate(lens):
        mk = torch.from_numpy(np.ascontiguousarray(irm_stack[:, fidx[u, 0]:fidx[u, 1]].T)).to(dev)
        y = ops.istft_masked(re_d[u][None], im_d[u][None], mk[None], n, N_fft, hop)
        c = torch.from_numpy(clean[u]).to(dev)[None]
        snr_d.append(float(ops.snr_db(y, c)[0])); sdr_d.append(float(ops.sdr_db(y, c, flen=32)[0]))
        wav_d.append(y[0].cpu().numpy())

    # ---- the same flow through the oracle ---------------------------------------------------
    w = model.get_weights()
    names = ["log_h0"] + list(model.cell._alt.keys()) + ["kc", "kn"]
    wd = dict(zip(names, w))
    alt = {k: wd[k] for k in model.cell._alt.keys()}
    for u, n in enumerate(lens):
        S = O.stft_mc(O.wav_int16_to_float(pcm[u]), N_fft, hop, win)
        xm = np.sqrt(S.real ** 2 + S.imag ** 2).T                             # (frames, F)
        np.testing.assert_allclose(stack[:F, fidx[u, 0]:fidx[u, 1]], S.real, atol=2e-5)
        # the model sees the utterance in maxlen-frame pieces, state restarting in every piece
        pieces = [xm[t:t + maxlen] for t in range(0, xm.shape[0], maxlen)]
        mk = np.concatenate([O.model_forward(pc[None], alt, model.cell.maps_from_alt.labels_per_k,
                                             K, wd["log_h0"], wd["kc"], wd["kn"],
                                             mask_value=-1.)[0][0] for pc in pieces])
        y = O.reconstruct(S.real, S.imag, mk.T, hop, win, nsampl=n)
        assert np.max(np.abs(wav_d[u] - y)) <= 1e-4 * max(np.max(np.abs(y)), 1e-3)
        assert abs(snr_d[u] - O.snr_db(y, clean[u].astype(np.float64))) <= 1e-2
        assert abs(sdr_d[u] - O.sdr_db(y, clean[u].astype(np.float64), 32)) <= 1e-2
    assert m.sum() == sum(nfr) and x.shape[0] == sum(-(-f // maxlen) for f in nfr)


# ------------------------------------------------------------------ KL / beta variant of the cell
def _run_ista_cell(dev, P, alt, labels, N, K, divergence, beta=1.5, return_all_hidden=False,
                   initial_state=None, want_state=False):
    from drnmf_amd import ops
    X = P["X"]
    B, T, F = X.shape
    stack = lambda name: np.stack([alt[k] for k in dict.fromkeys(labels[name])], 0)
    logD, logA, logL = stack("log_D"), stack("log_alph"), stack("log_lam1")
    desc = ops.make_desc(B, T, F, N, K, n_D=logD.shape[0], n_alph=logA.shape[0],
                         alph_len=int(np.asarray(logA[0]).size), n_lam=logL.shape[0],
                         return_all_hidden=return_all_hidden, divergence=divergence)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    params = ops.prepare_params(desc, t(logD), t(logA.reshape(logA.shape[0], -1)), t(logL.reshape(-1)))
    fin = torch.empty((B, N), dtype=torch.float32, device=dev) if want_state else None
    h = ops.cell_forward_ista(t(X), -1.0, params, desc, t(P["log_h0"]), beta=beta,
                              initial_state=t(initial_state), final_state=fin)
    torch.cuda.synchronize()
    return (h.cpu().numpy(), fin.cpu().numpy()) if want_state else h.cpu().numpy()


@pytest.mark.parametrize("cfg", [
    dict(B=3, T=6, F=21, r=6, K=3),
    dict(B=17, T=4, F=33, r=8, K=1),                          # K = 1, two row tiles
    dict(B=5, T=5, F=65, r=20, K=4, untied=()),               # tied, F = 16 k + 1 (no side path here)
    dict(B=4, T=3, F=513, r=100, K=2, untie_alph=True),
    dict(B=40, T=3, F=34, r=17, K=2, ragged=False),
    dict(B=250, T=2, F=513, r=1000, K=2, ragged=False, alph=400.0),      # row-blocked kernels
])
@pytest.mark.parametrize("divergence", ["kl", "beta"])
def test_kl_beta_cell_matches_oracle(dev, cfg, divergence):
    """The warm-started ISTA cell (drnmf_cell_forward_ista; the reference's ista_kl / ista_beta run
    recurrently, tests/test_oracle.py pins the restatement to them) against the fp64 oracle."""
    cfg = dict(cfg)
    K = cfg.pop("K")
    P, alt, labels, N = _problem(cfg.pop("B"), cfg.pop("T"), cfg.pop("F"), cfg.pop("r"), K,
                                 ragged=cfg.pop("ragged", True), density=0.3, **cfg)
    P["X"] = np.where(P["X"] == -1.0, -1.0, P["X"] + 0.05).astype(np.float32)   # keep x^ away from 0
    layers = O.maps_factored(alt, labels, K)
    for ah in (False, True):
        h = _run_ista_cell(dev, P, alt, labels, N, K, divergence, return_all_hidden=ah)
        ref = O.cell_forward_ista_warm(P["X"], layers, P["log_h0"], divergence=divergence,
                                       beta=1.5, return_all_hidden=ah)
        _check_h(h, ref)
    init = np.abs(np.random.default_rng(0).standard_normal((P["X"].shape[0], N))).astype(np.float32)
    h, fin = _run_ista_cell(dev, P, alt, labels, N, K, divergence, initial_state=init,
                            want_state=True)
    ref, rfin = O.cell_forward_ista_warm(P["X"], layers, P["log_h0"], divergence=divergence,
                                         beta=1.5, initial_state=init, return_state=True)
    _check_h(h, ref)
    _check_h(fin, rfin)


def test_kl_beta_cell_entry_points_are_kept_apart(dev):
    from drnmf_amd import ops
    P, alt, labels, N = _problem(2, 2, 21, 6, 2)
    with pytest.raises(ValueError):             # the reference cell's entry refuses a KL descriptor
        desc = ops.make_desc(2, 2, 21, N, 2, divergence="kl")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        prm = ops.prepare_params(desc, t(alt["log_D_0"][None]), t(alt["log_alph_0"].reshape(1, -1)),
                                 t(alt["log_lam1"].reshape(-1)))
        ops.cell_forward(t(P["X"]), -1.0, prm, desc, t(P["log_h0"]), (1.0, 0.0, 0.0))
    with pytest.raises(ValueError):             # and the ISTA entry refuses an ED descriptor
        desc = ops.make_desc(2, 2, 21, N, 2)
        prm = ops.prepare_params(desc, t(alt["log_D_0"][None]), t(alt["log_alph_0"].reshape(1, -1)),
                                 t(alt["log_lam1"].reshape(-1)))
        ops.cell_forward_ista(t(P["X"]), -1.0, prm, desc, t(P["log_h0"]))


def test_kl_cell_through_the_layer_surface(dev):
    """build_unfolded_snmf(..., divergence='kl') (extension key): the model predicts with the KL
    cell under the unchanged mask head and trains (gradients: tests/test_gpu_train.py)."""
    from drnmf_amd import layers
    B, T, F, r, K = 5, 7, 33, 10, 3
    P = O.synth_problem(B, T, F, r, seed=4, ragged=True, density=0.3)
    P["X"] = np.where(P["X"] == -1.0, -1.0, P["X"] + 0.05).astype(np.float32)
    N = 2 * r
    p = dict(input_dim=F, hidden_dim=N, output_dim=F, mask_value=-1., maxseq=T, K_layers=K,
             W=P["W"], alph=N / 4.0, lam1=0.3, params_untied=["log_D", "log_alph"],
             params_trainable=["log_D", "log_alph"], divergence="kl")
    model = layers.build_unfolded_snmf(p, device=dev)
    irm = model.predict_on_batch(P["X"])
    w = model.get_weights()
    names = ["log_h0"] + list(model.cell._alt.keys()) + ["kc", "kn"]
    wd = dict(zip(names, w))
    alt = {k: wd[k] for k in model.cell._alt.keys()}
    labels = model.cell.maps_from_alt.labels_per_k
    h = O.cell_forward_ista_warm(P["X"], O.maps_factored(alt, labels, K), wd["log_h0"],
                                 divergence="kl")
    ref, _, _ = O.head_forward(h, wd["kc"], wd["kn"])
    assert np.mean((irm - ref) ** 2) <= MASK_MSE_TOL
    model.compile(lr=1e-3)                       # the KL / beta cell has its own BPTT
    wmask = (P["X"] != -1.0).any(-1).astype(np.float32)
    assert np.isfinite(model.train_on_batch(P["X"], P["Y"], wmask))
    with pytest.raises(ValueError):
        layers.build_unfolded_snmf(dict(p, divergence="is"), device=dev)


def test_plain_c_host_program_over_the_c_abi(dev, tmp_path):
    """tests/c_abi/cell_smoke.c: a C99 host program (gcc, libamdhip64 + libdrnmf.so, no Python or
    torch in the process) runs prepare_params + cell_forward and reproduces the oracle."""
    import os
    import shutil
    import struct
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gcc = shutil.which("gcc")
    if gcc is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs gcc and the ROCm headers")
    K = 3
    P, alt, labels, N = _problem(5, 6, 33, 8, K, ragged=True)
    ref = _oracle_cell(P, alt, labels, K)
    B, T, F = P["X"].shape
    u = O.u_scalars(alt, np.float32)
    blob = struct.pack("<5i3ff", B, T, F, N, K, float(u[0]), float(u[1]), float(u[2]), -1.0)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).tobytes()
    blob += f32(P["X"]) + f32(np.stack([alt["log_D_%d" % k] for k in range(K)]))
    blob += f32(np.stack([alt["log_alph_%d" % k] for k in range(K)])) + f32(alt["log_lam1"])
    blob += f32(P["log_h0"]) + f32(ref)
    prob = tmp_path / "problem.bin"
    prob.write_bytes(blob)
    exe = str(tmp_path / "cell_smoke")
    libdir = os.path.join(root, "dr-nmf_amd")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "c_abi", "cell_smoke.c"), "-L/opt/rocm/lib",
                    "-lamdhip64", "-L" + libdir, "-ldrnmf", "-lm", "-Wl,-rpath,/opt/rocm/lib",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True)
    out = subprocess.run([exe, str(prob)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    err, mx = (float(out.stdout.split(k)[1].split()[0]) for k in ("max_abs_err", "max_ref"))
    assert mx > 0 and err <= H_TOL * mx, out.stdout
    # ... and the same host switches the handle's matrix mode (drnmf_set_matrix_mode): frame-parallel ISTA in the
    # exact-fp32 and the split-operand mode agree to fp32 rounding
    diff = float(out.stdout.split("max_rel_diff")[1].split()[0])
    assert diff <= 2e-5, out.stdout


def test_graph_cache_key_carries_the_layout_choices(dev, monkeypatch):
    """the cached frame graphs of a call are keyed by its pointers and shapes -- and by the layout
    choices baked into their nodes (row blocks, atom ranges).  Two calls with the SAME tensors (input, prepared
    block, output, workspace) under different row blockings -- what a sub-batch of a split call and a direct
    call of the same B can take, here forced through DRNMF_RB -- lay the workspace out differently (Bp = 48
    against 64 at B = 48): replaying the first call's graphs in the second would read the packed input with
    the wrong strides.  Both calls must match the oracle."""
    from drnmf_amd import ops
    monkeypatch.setenv("DRNMF_GRAM", "0")
    monkeypatch.setenv("DRNMF_SPLIT", "1")
    B, T, F, r, K = 48, 5, 33, 20, 3
    P, alt, labels, N = _problem(B, T, F, r, K, ragged=True, seed=3)
    stack = lambda name: np.stack([alt[k] for k in dict.fromkeys(labels[name])], 0)
    logD, logA, logL = stack("log_D"), stack("log_alph"), stack("log_lam1")
    desc = ops.make_desc(B, T, F, N, K, n_D=logD.shape[0], n_alph=logA.shape[0],
                         alph_len=int(np.asarray(logA[0]).size), n_lam=logL.shape[0])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    params = ops.prepare_params(desc, t(logD), t(logA.reshape(logA.shape[0], -1)), t(logL.reshape(-1)))
    x, h0 = t(P["X"]), t(P["log_h0"])
    u = O.u_scalars(alt, np.float32)
    sizes = []
    for rb in ("1", "2"):
        monkeypatch.setenv("DRNMF_RB", rb)
        sizes.append(ops.cell_workspace(desc, dev).numel())
    ws = torch.empty(max(sizes), dtype=torch.uint8, device=dev)
    out = torch.empty((B, T, N), dtype=torch.float32, device=dev)
    ref = O.cell_forward_factored(P["X"], O.maps_factored(alt, labels, K), O.u_scalars(alt), P["log_h0"],
                                  mask_value=-1.0)
    for rb in ("1", "2", "1"):
        monkeypatch.setenv("DRNMF_RB", rb)
        ops.cell_forward(x, -1.0, params, desc, h0, u, out=out, workspace=ws)
        torch.cuda.synchronize()
        _check_h(out.cpu().numpy(), ref)


@pytest.mark.parametrize("B,split,r,gram", [
    (100, None, 20, "0"), (100, "1", 20, "0"), (130, "3", 20, "0"), (250, "2", 20, "0"),
    (97, "4", 20, "0"), (200, "8", 20, "0"), (200, None, 250, None), (512, None, 20, "0")],
    ids=lambda v: "-" if v is None else str(v))
def test_large_batch_sub_batches_on_side_streams(dev, monkeypatch, B, split, r, gram):
    """Inference batches of 96 rows and more run as independent sub-batches on side streams of the handle
    (csrc/cell_shared.h Workspace::split; batch rows never interact, custom_layers.py:337-338, 346-348).
    Ragged lengths, a masked first frame in the LAST sub-batch, caller-supplied initial states and the
    final states read back: every sub-batch count (also uneven ones: 97 rows as 32+32+32+1, 130 as
    64+64+2) against the fp64 oracle, and the final state of every row against the oracle's.  Last case:
    N = 500 at B = 200 -- the whole batch is past the Gram form's size rule (factored, split), its 128- and
    72-row sub-batches are inside it: each sub-batch takes its own form.  B = 512: four sub-batches of 128."""
    from drnmf_amd import ops
    if gram is None:
        monkeypatch.delenv("DRNMF_GRAM", raising=False)
    else:
        monkeypatch.setenv("DRNMF_GRAM", gram)       # (the split serves the factored form)
    if split is None:
        monkeypatch.delenv("DRNMF_SPLIT", raising=False)
    else:
        monkeypatch.setenv("DRNMF_SPLIT", split)
    K, T, F = 3, 7, 33
    P, alt, labels, N = _problem(B, T, F, r, K, ragged=True, seed=B)
    P["X"][B - 1, 0] = -1.0
    rng = np.random.default_rng(B)
    init = np.abs(rng.standard_normal((B, N))).astype(np.float32) * (rng.random((B, N)) < 0.3)
    stack = lambda name: np.stack([alt[k] for k in dict.fromkeys(labels[name])], 0)
    logD, logA, logL = stack("log_D"), stack("log_alph"), stack("log_lam1")
    desc = ops.make_desc(B, T, F, N, K, n_D=logD.shape[0], n_alph=logA.shape[0],
                         alph_len=int(np.asarray(logA[0]).size), n_lam=logL.shape[0])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    params = ops.prepare_params(desc, t(logD), t(logA.reshape(logA.shape[0], -1)), t(logL.reshape(-1)))
    fin = torch.full((B, N), -7.0, dtype=torch.float32, device=dev)
    u = O.u_scalars(alt, np.float32)
    outs = []
    for _ in range(2):                               # (second call: the cached graphs of every sub-batch)
        h = ops.cell_forward(t(P["X"]), -1.0, params, desc, t(P["log_h0"]), u, initial_state=t(init),
                             final_state=fin)
        torch.cuda.synchronize()
        outs.append(h.cpu().numpy())
    ops.check_status(dev)
    assert np.array_equal(outs[0], outs[1])
    ref, st = O.cell_forward_factored(P["X"], O.maps_factored(alt, labels, K), O.u_scalars(alt), P["log_h0"],
                                      mask_value=-1.0, initial_state=init.astype(np.float64), return_state=True)
    _check_h(outs[0], ref)
    np.testing.assert_allclose(fin.cpu().numpy(), st, atol=H_TOL * max(np.max(np.abs(st)), 1e-30))


@pytest.mark.parametrize("K", [3, 1])
def test_cell_profile_leaves_the_forward_s_output(dev, monkeypatch, K):
    """drnmf_cell_profile (bench.py, tools/profile_shape.py) launches the factored chain directly, a HIP event
    ahead of every launch: the same kernels on the same arguments as the graphs of drnmf_cell_forward.  All T
    frames must leave the forward's output bit for bit, two frames its first two; the three times come back
    finite, the frame's positive.  K = 1: one cell_a launch and the frame-counter advance per frame.  The
    entry brackets the factored launches only: a call that takes the Gram form is refused (-2)."""
    from drnmf_amd import ops
    monkeypatch.setenv("DRNMF_GRAM", "0")
    B, T, F, r = 20, 6, 33, 20
    P, alt, labels, N = _problem(B, T, F, r, K, ragged=True)
    stack = lambda name: np.stack([alt[k] for k in dict.fromkeys(labels[name])], 0)
    logD, logA, logL = stack("log_D"), stack("log_alph"), stack("log_lam1")
    desc = ops.make_desc(B, T, F, N, K, n_D=logD.shape[0], n_alph=logA.shape[0],
                         alph_len=int(np.asarray(logA[0]).size), n_lam=logL.shape[0])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    params = ops.prepare_params(desc, t(logD), t(logA.reshape(logA.shape[0], -1)), t(logL.reshape(-1)))
    x, h0 = t(P["X"]), t(P["log_h0"])
    u = O.u_scalars(alt, np.float32)
    nbytes = ops.cell_workspace(desc, dev).numel()
    ws = lambda: torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    ref = ops.cell_forward(x, -1.0, params, desc, h0, u, workspace=ws())
    torch.cuda.synchronize()
    ref = ref.cpu().numpy()
    for frames in (T, 2):
        out = torch.full((B, T, N), -7.0, dtype=torch.float32, device=dev)
        us = ops.cell_profile(x, -1.0, params, desc, h0, u, out, ws(), frames=frames)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy()[:, :frames], ref[:, :frames]), frames
        assert all(np.isfinite(us[k]) for k in ("cell_a_us", "cell_b_us", "frame_us")), us
        assert us["frame_us"] > 0, us
    if K >= 2:                                       # (K = 1 never takes the Gram form)
        monkeypatch.setenv("DRNMF_GRAM", "1")
        out = torch.empty((B, T, N), dtype=torch.float32, device=dev)
        unsupported = -2                             # DRNMF_ERR_UNSUPPORTED (include/drnmf.h)
        with pytest.raises(ValueError, match=r"drnmf_cell_profile failed \(%d\)" % unsupported):
            ops.cell_profile(x, -1.0, params, desc, h0, u, out, ops.cell_workspace(desc, dev), frames=T)
    ops.check_status(dev)


def test_split_call_refuses_a_sub_batch_that_outgrows_its_slice(dev, monkeypatch):
    """The slices of a split call's workspace are sized for a sub-batch of split_rows rows.  A smaller LAST
    sub-batch may take the Gram form (its size rule grows with the batch), and the Gram form's ring of hoisted
    c_k is far larger than a factored slice: B = 160, N = 1000 runs as 64 + 64 factored rows and 32 Gram rows
    whose layout ends tens of MB past the workspace drnmf_cell_workspace_bytes asks for.  Such a call must come
    back with DRNMF_ERR_WORKSPACE, before anything of that sub-batch is enqueued, and leave the handle usable."""
    from drnmf_amd import ops
    monkeypatch.delenv("DRNMF_GRAM", raising=False)
    monkeypatch.delenv("DRNMF_SPLIT", raising=False)
    B, T, F, N, K = 160, 8, 257, 1000, 5
    desc = ops.make_desc(B, T, F, N, K, n_D=K, n_alph=K)
    rng = np.random.default_rng(0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    params = ops.prepare_params(desc, t(np.log(rng.random((K, F, N)) + 0.1)), t(np.full((K, 1), np.log(N / 4.0))),
                                t(np.full((1,), np.log(0.3))))
    x, h0 = t(rng.random((B, T, F))), t(np.zeros(N))
    workspace_err = -4                               # DRNMF_ERR_WORKSPACE (include/drnmf.h)
    with pytest.raises(ValueError, match=r"drnmf_cell_forward failed \(%d\): cell_forward: workspace" % workspace_err):
        ops.cell_forward(x, -1.0, params, desc, h0, (1.0, 0.0, 0.0))
    torch.cuda.synchronize()
    ops.check_status(dev)
    small = ops.make_desc(32, T, F, N, K, n_D=K, n_alph=K)          # the same rows as a call of their own: fine
    h = ops.cell_forward(x[:32].contiguous(), -1.0, params, small, h0, (1.0, 0.0, 0.0))
    torch.cuda.synchronize()
    assert np.all(np.isfinite(h.cpu().numpy()))
