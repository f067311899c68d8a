"""tests/drnmf_train_ref.py on the CPU: the stage references against autograd of the whole model_loss, relu_margin on a
constructed kink, and the restated selection rules at shapes worked out BY HAND from csrc/gemm_tn.h,
csrc/cell_shared.h, csrc/cell_backward.hip and csrc/train.hip (the values tests/test_gpu_train_edges.py relies on)."""
import numpy as np
import pytest
import torch

from oracle import drnmf_oracle as O
from oracle import drnmf_torch_ref as TR

import drnmf_train_ref as R


def _problem(B=4, T=6, F=21, r=5, K=3, seed=3, divergence="ed", untied=("log_D", "log_alph", "log_lam1")):
    P = O.synth_problem(B, T, F, r, seed=seed, ragged=True, density=0.3)
    N = 2 * r
    if divergence != "ed":
        P["X"] = np.where(P["X"] == -1.0, -1.0, P["X"] + 0.1).astype(np.float32)
    P["X"][1, :2] = -1.0                                  # a row that starts masked
    params = dict(W=P["W"], U1=np.eye(N, dtype=np.float32), Uk=np.zeros((N, N), np.float32),
                  alph=np.float32(N / 4.0 if divergence == "ed" else 2.0 * N),
                  lam1=np.float32(0.3 if divergence == "ed" else 0.05))
    alt, labels = O.build_alt(N, K, params, untied)
    rng = np.random.default_rng(seed)
    for k in list(alt):
        if k.startswith(("log_D", "log_alph", "log_lam1")):
            alt[k] = (alt[k] + 0.05 * rng.standard_normal(np.shape(alt[k]))).astype(np.float32)
    kc = (0.3 * rng.standard_normal((r, F))).astype(np.float32)
    kn = (0.3 * rng.standard_normal((r, F))).astype(np.float32)
    w = (P["X"] != -1.0).any(-1).astype(np.float64)
    w[0, 0], w[2, 1] = 0.0, 0.5
    return P, alt, labels, N, K, kc, kn, w


def _whole(P, alt, labels, K, kc, kn, w, square=False, l1=None, divergence="ed", init=None):
    """Autograd of model_loss: (loss, {name: grad}, hs, d loss / d hs)."""
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    leaves = {k: t64(v).requires_grad_(True) for k, v in alt.items()}
    lh0, tkc, tkn = (t64(v).requires_grad_(True) for v in (P["log_h0"], kc, kn))
    x = t64(P["X"])
    loss, mask, hs = TR.model_loss(x, x if l1 is not None else t64(P["Y"]), t64(w), leaves, labels, K, lh0, tkc, tkn,
                                   square=square, normalise=False, snmf_cost_l1_weight=l1, divergence=divergence,
                                   initial_state=None if init is None else t64(init))
    hs.retain_grad()
    loss.backward()
    z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    g = {k: z(v) for k, v in leaves.items()}
    g.update(log_h0=z(lh0), kc=z(tkc), kn=z(tkn))
    return float(loss.detach()), g, hs.detach().numpy(), hs.grad.numpy()


@pytest.mark.parametrize("divergence,stateful", [("ed", False), ("kl", False), ("ed", True), ("beta", True)])
def test_cell_vjp_with_the_heads_cotangent_reproduces_model_loss(divergence, stateful):
    P, alt, labels, N, K, kc, kn, w = _problem(divergence=divergence)
    init = 0.1 + 0.2 * np.random.default_rng(1).random((P["X"].shape[0], N)) if stateful else None
    _, g, hs, cot = _whole(P, alt, labels, K, kc, kn, w, divergence=divergence, init=init)
    got = R.cell_vjp(P["X"], alt, labels, K, P["log_h0"], cot, initial_state=init, divergence=divergence)
    assert set(got) == set(alt) | {"log_h0"}
    for n in got:
        np.testing.assert_allclose(got[n], g[n], rtol=1e-12, atol=1e-14 * max(np.abs(g[n]).max(), 1e-30), err_msg=n)
    assert np.abs(got[labels["log_D"][0]]).max() > 0
    if stateful:
        assert not got["log_h0"].any()                    # unused: zeros, not None
    else:
        assert got["log_h0"].any()
    # the fp32 yardstick runs the same graph
    g32 = R.cell_vjp(P["X"], alt, labels, K, P["log_h0"], cot, initial_state=init, divergence=divergence,
                     dtype=torch.float32)
    n = labels["log_D"][K - 1]
    err = np.abs(g32[n] - got[n]).max() / np.abs(got[n]).max()
    assert 0 < err < 1e-3


def test_cell_vjp_without_a_valid_frame_is_zero():
    P, alt, labels, N, K, _, _, _ = _problem()
    x = np.full_like(P["X"], -1.0)
    got = R.cell_vjp(x, alt, labels, K, P["log_h0"], np.ones(x.shape[:2] + (N,)))
    assert all(not v.any() for v in got.values())


@pytest.mark.parametrize("square", [False, True])
def test_head_functions_equal_autograd_of_model_loss(square):
    P, alt, labels, N, K, kc, kn, w = _problem()
    loss, g, hs, cot = _whole(P, alt, labels, K, kc, kn, w, square=square)
    F = P["X"].shape[-1]
    flat = lambda a: np.asarray(a).reshape(-1, a.shape[-1])
    s, c, dh, dkc, dkn = R.head_loss_and_grads(flat(P["X"]), flat(hs), kc, kn, flat(P["Y"]), w.reshape(-1), square)
    assert abs(s - loss) <= 1e-12 * abs(loss) and c == float((w != 0).sum())
    np.testing.assert_allclose(dh, flat(cot), rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(dkc, g["kc"], rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(dkn, g["kn"], rtol=1e-12, atol=1e-18)
    m, A, Bn = R.head_forward_ref(flat(hs), kc, kn, square)
    assert m.shape == (hs.shape[0] * hs.shape[1], F) and (m >= 0).all() and (m <= 1).all()
    np.testing.assert_allclose(m, (1e-7 + A) / (1e-7 + A + Bn), rtol=1e-12)
    if not square:
        l1 = 0.3 * N / F
        loss, g, hs, cot = _whole(P, alt, labels, K, kc, kn, w, l1=l1)
        s, c, dh, dkc, dkn = R.snmf_cost_head_grads(flat(P["X"]), flat(hs), kc, kn, w.reshape(-1), l1)
        assert abs(s - loss) <= 1e-12 * abs(loss) and c == float((w != 0).sum())
        np.testing.assert_allclose(dh, flat(cot), rtol=1e-12, atol=1e-18)
        np.testing.assert_allclose(dkc, g["kc"], rtol=1e-12, atol=1e-18)
        np.testing.assert_allclose(dkn, g["kn"], rtol=1e-12, atol=1e-18)


def test_relu_margin_is_zero_on_a_constructed_kink():
    """K = 1, one valid frame, p = softplus(log_h0): the pre-activation of atom n is u0d p[n] + u0o (sum(p) - p[n]) +
    (x Dn)[n] / alpha - lam / alpha.  lam is set so that atom 2 of row 0 vanishes: margin 0 with row 0 selected,
    > 0 on row 1."""
    P, alt, labels, N, K, _, _, _ = _problem(K=1, untied=())
    x = P["X"][[0, 2], :1].copy()
    assert (x != -1.0).any(-1).all()
    lh0 = P["log_h0"].astype(np.float64)
    alt = {k: np.asarray(v, np.float64) for k, v in alt.items()}
    assert R.relu_margin(x, alt, labels, 1, lh0) > 1e-6
    D = np.exp(alt["log_D"])
    Dn = D / np.sqrt((D * D).sum(0))
    ia = np.exp(-float(alt["log_alph"]))
    U1 = np.exp(alt["log_U1"])
    p = np.log1p(np.exp(lh0))
    base = U1[0, 0] * p[2] + U1[0, 1] * (p.sum() - p[2]) + (x[0, 0].astype(np.float64) @ Dn)[2] * ia
    alt["log_lam1"] = np.log(base / ia)
    assert R.relu_margin(x, alt, labels, 1, lh0, rows=[0]) < 1e-12
    assert R.relu_margin(x, alt, labels, 1, lh0) < 1e-12
    assert R.relu_margin(x, alt, labels, 1, lh0, rows=[1]) > 1e-6
    x[1] = -1.0                                                                 # no valid frame in the selection
    assert R.relu_margin(x, alt, labels, 1, lh0, rows=[1]) == float("inf")


# ---- the restated rules at hand-computed shapes ---------------------------------------------------------------

def test_split_rules_by_hand():
    # gemm_tn::pick_splits: splits while rows / s >= 192, cost ceil(tiles s / 512) / s (1 + 0.004 s); k-tiles of 32
    assert R.tn_plan(32, 12, 1540) == (8, [7])          # 49 k-tiles, 7 per split: split 7 empty; last tile 4 rows
    assert R.tn_plan(32, 12, 416) == (2, [])            # 13 k-tiles: 7 + 6
    assert R.tn_plan(32, 12, 383) == (1, [])
    assert R.tn_plan(32, 12, 384) == (2, [])
    assert R.tn_plan(32, 260, 390) == (2, [])
    assert R.tn_plan(32, 516, 390) == (2, [])
    assert R.tn_plan(2048, 12, 6) == (1, [])
    assert R.bptt_gemm_m(33) == 32 and R.bptt_gemm_m(34) == 48 and R.bptt_gemm_m(21) == 32
    assert R.bptt_gemm_m(33, "kl") == 48 and R.bptt_gemm_m(17) == 16 and R.bptt_gemm_m(16) == 16
    assert R.odd_bin(33) and R.odd_bin(257) and not R.odd_bin(34) and not R.odd_bin(1) and not R.odd_bin(33, "kl")
    # the heads: pick_splits(r, Fp4, rows, 64)
    assert R.head_plan(1540, 33, 6) == (36, 385, 8, [7])
    assert R.head_plan(1023, 21, 3) == (24, 256, 5, [])
    assert R.head_plan(1025, 16, 4) == (16, 257, 5, [])
    assert R.head_plan(5, 5, 1) == (8, 2, 1, [])
    assert R.head_plan(4, 257, 17) == (260, 1, 1, [])


def test_column_reduction_rules_by_hand():
    assert R.CR_SPLITS == 256
    assert R.cr_split_rows(0, 1540) == (0, 7) and R.cr_split_rows(31, 1540) == (217, 224)
    assert R.cr_split_rows(219, 1540) == (1533, 1540) and R.cr_split_rows(220, 1540)[0] >= 1540
    assert R.cr_split_of(220, 1540) == 31 and R.cr_split_of(219, 1540) == 31 and R.cr_split_of(216, 1540) == 30
    assert R.cr_split_rows(207, 416) == (414, 416) and R.cr_split_rows(3, 6) == (3, 4)
    assert [R.colreduce_form(n) for n in (12, 14, 256, 260, 516, 7, 33)] == \
        [(4, 4, 4), (1, 1, 8), (4, 4, 4), (4, 1, 4), (4, 1, 4), (1, 1, 8), (1, 1, 8)]
    assert [R.fold_form(n) for n in (12, 260, 512, 516)] == [4, 4, 4, 1]
    assert R.dlogd_form(33, 12) == ("vec", 1, 9)
    assert R.dlogd_form(2040, 12) == ("vec", 4, 128)      # 1 x 128 tiles of 16 bins: not < 128
    assert R.dlogd_form(2024, 12) == ("vec", 1, 506)      # 127 tiles
    assert R.dlogd_form(65, 12) == ("vec", 1, 17)
    assert R.dlogd_form(21, 12) == ("vec", 1, 6)
    assert R.dlogd_form(33, 14) == ("scalar", 0, 0)
    assert R.dlogd_form(513, 2000) == ("vec", 4, 33)      # 8 x 33 = 264 workgroups


def test_cell_rules_by_hand():
    assert [R.ntail_of(F) for F in (15, 16, 17, 18, 19, 21, 33, 34, 35, 257, 2040)] == [0, 0, 1, 2, 0, 0, 1, 2, 0, 1, 0]
    assert R.ntail_of(33, "kl") == 0
    assert [R.nft_main_of(F) for F in (15, 17, 19, 33, 34, 35, 257)] == [1, 1, 2, 2, 2, 3, 16]
    # atom ranges: doubled while tiles KS < 192 and (Np / 16) / (2 KS) >= 4, at most 4
    assert R.ks_of(3, 33, 16) == (1, 2)
    assert R.ks_of(3, 33, 130) == (2, 5)                  # Np = 160: 10 chunks
    assert R.ks_of(3, 33, 260) == (4, 5)                  # Np = 288: 18 chunks in ranges of 5, 5, 5, 3
    assert R.ks_of(3, 33, 340, env=8) == (8, 3)           # Np = 352: 22 chunks in ranges of 3 x 7, 1
    assert R.ks_of(3, 257, 2080) == (4, 33)               # Np = 2080: 130 chunks; 16 tiles x 4 = 64 < 192
    assert R.ks_of(64, 513, 2000) == (2, 63)              # the headline shape: 4 x 32 tiles, 128 -> 256 workgroups
    assert R.ks_of(3, 33, 260, divergence="kl") == (1, 18)
    assert R.rb_of(3, 33, 16) == 1 and R.rb_of(1, 33, 16, env=2) == 2 and R.rb_of(250, 513, 2000) == 2
    assert R.rb_of(250, 513, 2000, gram=True) == 1
    assert R.ks_of(17, 33, 16, rb_env=2) == (1, 2)
    # qred: an odd bin, more than 64 atom blocks, nft KS >= 16 RB
    assert R.qred_of(3, 257, 2080) and not R.qred_of(3, 257, 2000) and not R.qred_of(3, 256, 2080)
    assert not R.qred_of(3, 33, 2080)                     # 2 bin tiles x 4 ranges < 16
    assert R.gram_of(3, 16, 3) and not R.gram_of(3, 16, 1) and not R.gram_of(3, 16, 3, env=0)
    assert not R.gram_of(3, 2080, 2) and R.gram_of(3, 2080, 2, env=1) and not R.gram_of(3, 16, 3, divergence="kl")
    assert R.gram_of(16, 1000, 3) and not R.gram_of(64, 1000, 3)          # 1 and 4 row tiles x 1024^2 against 3e6
    # frames per graph: 800 kernel nodes at 2 K - 1 launches a frame, 1 .. 64, at most T
    assert R.frames_per_graph(7, 200) == 61 and R.frames_per_graph(2, 200) == 64 and R.frames_per_graph(7, 60) == 60
    assert R.frames_per_graph(25, 2000) == 16 and R.frames_per_graph(1, 5) == 5 and R.frames_per_graph(500, 9) == 1


def test_the_split_rules_are_the_lstm_suites_own():
    import test_gpu_lstm_train_edges as L
    assert R.pick_splits is L.pick_splits and R.empty_splits is L.empty_splits
