"""The stage-wise fp64 helpers of tests/lstm_train_ref.py (head_loss_and_grads, hidden_vjp, kink_margin) against
the whole-model loss_and_grads they must agree with, and kink_margin on an input built to sit on a kink.  No GPU."""
import numpy as np
import torch

import lstm_ref as R
import lstm_state_ref as SR
import lstm_train_ref as TR


def _rel(a, b):
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


def _case(seed, B, T, F, H, K):
    rng = np.random.default_rng(seed)
    x, valid = R.masked_input(rng, B, T, F)
    y = rng.random((B, T, F)).astype(np.float32)
    w = valid.astype(np.float32)
    w[rng.random((B, T)) < 0.2] = 0.5                      # masked frames with weight among them
    w[rng.random((B, T)) < 0.1] = 0.0
    return rng, x, y, w, R.random_weights(rng, F, H, K, scale=1.5)


def _composed(x, y, w, wt, K, act, state=None):
    ks, rs, bs = wt[0:3 * K:3], wt[1:3 * K:3], wt[2:3 * K:3]
    ih, ic = state if state is not None else (None, None)
    hs, _, _ = SR.lstm_layers(x, ks, rs, bs, -1.0, act, ih, ic)
    xs = torch.as_tensor(x, dtype=torch.float64)
    xm = xs * R.valid_frames(xs, -1.0).unsqueeze(-1)
    loss, cnt, d_h, d_wo, d_bo = TR.head_loss_and_grads(xm, hs[-1], y, w, wt[-2], wt[-1])
    return loss, cnt, TR.hidden_vjp(x, wt, K, d_h, -1.0, act, state) + [d_wo, d_bo]


def test_head_composed_with_hidden_vjp_is_loss_and_grads():
    """(B, T, F, H, K) = (8, 9, 7, 5, 2), every mask pattern: the head's gradient pushed through hidden_vjp is the
    model's gradient to 1e-12, in both activations."""
    B, T, F, H, K = 8, 9, 7, 5, 2
    for act in ("hard_sigmoid", "sigmoid"):
        _, x, y, w, wt = _case(3, B, T, F, H, K)
        loss, cnt, gs = _composed(x, y, w, wt, K, act)
        loss_r, cnt_r, gr = TR.loss_and_grads(x, y, w, wt, K, -1.0, act)
        assert cnt == cnt_r and abs(loss - loss_r) <= 1e-12 * abs(loss_r)
        assert len(gs) == len(gr) == 3 * K + 2
        for g, r in zip(gs, gr):
            assert g.shape == r.shape and _rel(g, r) <= 1e-12


def test_hidden_vjp_with_an_entering_state_is_the_state_reference():
    B, T, F, H, K = 4, 6, 5, 3, 2
    rng, x, y, w, wt = _case(4, B, T, F, H, K)
    st = SR.random_state(rng, K, B, H)
    loss, cnt, gs = _composed(x, y, w, wt, K, "hard_sigmoid", st)
    loss_r, cnt_r, gr, _ = SR.loss_and_grads(x, y, w, wt, K, state=st)
    assert cnt == cnt_r and abs(loss - loss_r) <= 1e-12 * abs(loss_r)
    for g, r in zip(gs, gr):
        assert _rel(g, r) <= 1e-12


def test_hidden_vjp_of_an_all_masked_batch_is_zero():
    wt = R.random_weights(np.random.default_rng(0), 3, 2, 1)
    x = np.full((2, 4, 3), -1.0, np.float32)
    for g in TR.hidden_vjp(x, wt, 1, np.ones((2, 4, 2))):
        assert not g.any()
    assert TR.kink_margin(x, wt, 1) == float("inf")


def test_kink_margin_is_zero_on_a_kink_and_positive_off_it():
    """All weights zero, so z = bias at every frame: the bias of unit 1's forget gate at -2.5 puts 0.2 z + 0.5 on
    0 exactly, the output gate's at 2.5 on 1; the candidate gate (tanh) does not count; a masked row's kink does
    not count either."""
    F, H, K = 3, 2, 2
    x = np.full((2, 3, F), 0.25, np.float32)
    zero = [np.zeros_like(v) for v in R.random_weights(np.random.default_rng(0), F, H, K)]
    assert abs(TR.kink_margin(x, zero, K) - 0.5) <= 1e-15
    for layer, col, v in ((0, H + 1, -2.5), (1, 3 * H + 1, 2.5), (1, 0, -2.5)):
        wt = [a.copy() for a in zero]
        wt[3 * layer + 2][col] = v
        assert TR.kink_margin(x, wt, K) == 0.0
    wt = [a.copy() for a in zero]
    wt[2][2 * H] = 2.5                                      # the candidate gate: no kink there
    assert abs(TR.kink_margin(x, wt, K) - 0.5) <= 1e-15
    wt[2][0] = 2.0                                          # 0.2 * 2 + 0.5 = 0.9: 0.1 from the upper kink
    assert abs(TR.kink_margin(x, wt, K) - 0.1) <= 1e-15
    # the recurrent term counts: z_i(t >= 1) = U h_{t-1}, so a margin computed without it would differ
    rng = np.random.default_rng(1)
    wr = R.random_weights(rng, F, 8, 1, scale=1.5)
    xr = rng.random((2, 12, F)).astype(np.float32)
    m_full = TR.kink_margin(xr, wr, 1)
    wr0 = [a.copy() for a in wr]
    wr0[1][:] = 0
    assert m_full != TR.kink_margin(xr, wr0, 1) and m_full > 0
    rows = [TR.kink_margin(xr[b:b + 1], wr, 1) for b in range(2)]
    assert abs(min(rows) - m_full) <= 1e-15
    xm = xr.copy()
    xm[int(np.argmin(rows))] = -1.0                         # the closer row masked: the other one's margin
    assert abs(TR.kink_margin(xm, wr, 1) - max(rows)) <= 1e-15


PROBE = r"""
#include "gemm_tn.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
    for (int i = 1; i + 2 < argc; i += 3)
        std::printf("%d\n", gemm_tn::pick_splits(std::atoi(argv[i]), std::atoi(argv[i + 1]), std::atoll(argv[i + 2]), 32));
    return 0;
}
"""


def test_split_mirror_of_the_gpu_module_is_the_headers_rule(tmp_path):
    """tests/test_gpu_lstm_train_edges.py restates gemm_tn::pick_splits to name its cases; here the header's own
    function (host code, compiled into a probe) answers the same questions.  (lstm_colsum's rule sits inside
    lstm.hip's driver and has no such probe.)"""
    import importlib.util
    import os
    import subprocess
    import pytest
    import test_gpu_lstm_train_edges as E
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("drnmf_build_probe", os.path.join(root, "dr-nmf_amd", "build.py"))
    bm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bm)
    if not os.path.exists(bm.HIPCC):
        pytest.skip("no hipcc")
    src, exe = str(tmp_path / "probe.cpp"), str(tmp_path / "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.run([bm.HIPCC] + bm.ARCH + ["-x", "hip", "-std=c++17", "-O0", "-I", bm.CSRC, "-I",
                                           os.path.join(root, "include"), "-o", exe, src], check=True)
    qs = [(M, N, rows) for M in (4, 16, 40, 252, 516) for N in (20, 160, 516, 1024)
          for rows in (1, 191, 383, 384, 385, 400, 575, 576, 760, 779, 2040, 6143, 6144, 6400, 6435, 100000)]
    out = subprocess.run([exe] + [str(v) for q in qs for v in q], check=True, capture_output=True, text=True).stdout
    got = [int(v) for v in out.split()]
    assert len(got) == len(qs)
    for q, g in zip(qs, got):
        assert E.pick_splits(*q) == g, q
    assert set(got) >= {1, 2, 3, 10, 32}
