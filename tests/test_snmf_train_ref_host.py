"""tests/snmf_train_ref.py pinned on the CPU: the reference against a second restatement, the selection rules against
values worked out by hand from csrc/snmf.hip and csrc/gemm_tn.h, the float32 yardstick against the bounds, and the
bounds against mutants -- small variants of the one-step reference, each a mistake one of the dictionary-training
kernels could make at a branch the cases were chosen for.  tests/test_gpu_snmf_train_edges.py holds the device to the
same bounds."""
import numpy as np
import pytest

import snmf_train_ref as R


# ---- one iteration, restated ------------------------------------------------------------------------------------

def _one_step(V, W0, H0, sparsity, beta, case, mutant=None, flr=1e-9):
    """ONE iteration of sparse_nmf_gpu.m in float64 from the inputs, every atom updated: the few lines of
    tests/test_gpu_x3._snmf_step64 in numpy and the oracle's layout (V (F,n), W (F,N), H (N,n); beta 1 or 2), with
    the zeros of V floored as the oracle does.  mutant: one of MUTANTS, the place where it departs marked below.
    Returns W, H, [div], [cost]."""
    n, F, N = case
    V, W, H = (np.array(a, dtype=np.float64) for a in (V, W0, H0))
    if beta != 2.0:
        V[V == 0] = V[V > 0].min()
    wn = np.sqrt((W * W).sum(0))
    W, H = W / wn, H * wn[:, None]
    lam = np.maximum(W @ H, flr)
    if beta == 1.0:
        colsum = W.sum(0)
        if mutant == "h_update_takes_colsums_of_unnormalised_W0":
            colsum = np.asarray(W0, np.float64).sum(0)
        H = H * (W.T @ (V / lam)) / np.maximum(colsum[:, None] + sparsity, flr)
    else:
        H = H * (W.T @ V) / np.maximum(W.T @ lam + sparsity, flr)
    lam = np.maximum(W @ H, flr)
    src = V / lam if beta == 1.0 else V
    num = src @ H.T
    if beta == 1.0:
        hs = H.sum(1)
        if mutant == "hs_without_the_remainder_frames":
            hs = np.zeros(N)
            per = R.hs_per(n)
            for s in range(R.HS_SPLITS):
                a, b = min(s * per, n), min((s + 1) * per, n)
                hs += H[:, a:a + (b - a) // 8 * 8].sum(1)
        den = np.broadcast_to(hs[None, :], num.shape).copy()
    else:
        den = lam @ H.T
    r0, r1 = R.row_regions(F)
    if mutant == "num_tail_without_the_last_frame":
        num[r0:r1] -= np.outer(src[r0:r1, n - 1], H[:, n - 1])
    if mutant == "num_tail_with_the_last_frame_twice":
        num[r0:r1] += np.outer(src[r0:r1, n - 1], H[:, n - 1])
    if mutant == "den_without_the_last_split":
        ns = R.nsplit(n, R.Mg(F), N)
        a, b = [fr for fr in (R.split_frames(n, ns, s) for s in range(ns)) if fr[0] < fr[1]][-1]
        m = min(R.Mg(F), F)
        den[:m] -= lam[:m, a:b] @ H[:, a:b].T
    if mutant == "last_tail_row_takes_row_0s_sums":
        num[r1 - 1], den[r1 - 1] = num[r0], den[r0]
    Wold = W
    dpw = np.maximum(den + (num * W).sum(0, keepdims=True) * W, flr)
    W = W * (num + (den * W).sum(0, keepdims=True) * W) / dpw
    if mutant == "atoms_from_256_keep_their_W":
        W[:, R.ATOMS_PER_WG:] = Wold[:, R.ATOMS_PER_WG:]
    W = W / np.sqrt((W * W).sum(0))
    lam = np.maximum(W @ H, flr)
    terms = V * np.log(V / lam) - V + lam if beta == 1.0 else (V - lam) ** 2
    if mutant == "objective_without_the_last_bin":
        terms = terms[:F - 1]
    if mutant == "objective_without_the_last_row_tile_of_frames":
        terms = terms[:, :(n - 1) // R.OBJ_ROWS * R.OBJ_ROWS]
    div = terms.sum()
    return W, H, np.array([div]), np.array([div + sparsity * H.sum()])


# mutant -> (betas, the cases it can show at, the entry of errors() that must reject it)
_TAIL = [c for c, s in R.CASES.items() if R.tail_rows(s[1])]
_SPLIT = [c for c, s in R.CASES.items() if R.nsplit(s[0], R.Mg(s[1]), s[2]) > 1]
_WIDE = [c for c, s in R.CASES.items() if s[2] > R.ATOMS_PER_WG]
_ALL = list(R.CASES)
# (B's and C's 64 ranges of 16 frames, 40 in the last, leave colsum_rows_kernel's remainder loop nothing to do)
_REMAINDER = [c for c, s in R.CASES.items() if R.hs_per(s[0]) % 8 or (s[0] % R.hs_per(s[0])) % 8]
MUTANTS = {
    "num_tail_without_the_last_frame": ((2.0, 1.0), _TAIL, "W[rows"),
    "num_tail_with_the_last_frame_twice": ((2.0, 1.0), _TAIL, "W[rows"),
    "den_without_the_last_split": ((2.0,), _SPLIT, "W"),
    "last_tail_row_takes_row_0s_sums": ((2.0, 1.0), [c for c in _TAIL if R.tail_rows(R.CASES[c][1]) > 1], "W[rows"),
    "atoms_from_256_keep_their_W": ((2.0, 1.0), _WIDE, "W[atoms >="),
    "hs_without_the_remainder_frames": ((1.0,), _REMAINDER, "W"),
    "h_update_takes_colsums_of_unnormalised_W0": ((1.0,), _ALL, "H"),
    "objective_without_the_last_bin": ((2.0, 1.0), _ALL, "div"),
    "objective_without_the_last_row_tile_of_frames": ((2.0, 1.0), _ALL, "div"),
}

_REFS = {}


def _unmutated(c, beta):
    """One reference per (case, beta), shared by the mutants (and never modified)."""
    if (c, beta) not in _REFS:
        V, W0, H0 = R.problem(R.CASES[c], beta)
        _REFS[c, beta] = (V, W0, H0, _one_step(V, W0, H0, R.SPARSITY, beta, R.CASES[c]))
    return _REFS[c, beta]


# ---- the tests --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("beta", [1.0, 2.0])
def test_step_reference_agrees_with_the_second_restatement(beta):
    case = R.CASES["A"]
    V, W0, H0, mine = _unmutated("A", beta)
    ref = R.step_reference(V, W0, H0, R.SPARSITY, 1, beta, None)
    e = R.errors(mine, ref, case)
    print("A beta %g: %s" % (beta, R.fmt(e)))
    assert all(float(np.max(v)) <= 1e-12 for v in e.values()), e


def test_step_reference_switches():
    """update_w=False is the oracle with an all-false mask; W is then the normalised W0, whatever mask came with it."""
    case = R.CASES["G"]
    V, W0, H0 = R.problem(case, 2.0)
    a = R.step_reference(V, W0, H0, R.SPARSITY, 2, 2.0, R.w_ind(3, "thirds"), update_w=False)
    b = R.step_reference(V, W0, H0, R.SPARSITY, 2, 2.0, R.w_ind(3, "none"))
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    W0n = W0.astype(np.float64) / np.sqrt((W0.astype(np.float64) ** 2).sum(0))
    np.testing.assert_array_equal(a[0], W0n)
    assert a[2].shape == (2,) and a[3].shape == (2,)
    f32 = R.step_reference(V, W0, H0, R.SPARSITY, 1, 2.0, None, dtype=np.float32)
    assert f32[0].dtype == np.float32 and f32[1].dtype == np.float32
    np.testing.assert_array_equal(R.w_ind(7, "thirds"), [False, True, True, False, True, True, False])
    assert R.w_ind(7, None) is None and not R.w_ind(7, "none").any()


# worked out by hand from csrc/snmf.hip (tr_splits, tn_tail_rows, tn_tail_kernel, colsum_rows_kernel, the w_* grid)
# and csrc/gemm_tn.h (pick_splits: with tiles x splits <= 512 the cost 1/s + 0.004 falls with s, so the count is the
# largest s <= 64 with n // s >= 192)
EXPECTED = {
    #     nsplit tail Mg  tail_per hs_per w_groups atom_columns
    "A": (1, 0, 68, 1, 5, 9, 1),
    "B": (5, 2, 128, 2, 16, 17, 2),
    "C": (5, 3, 128, 2, 16, 17, 1),
    "D": (21, 1, 128, 9, 66, 17, 1),
    "E": (4, 4, 128, 2, 13, 17, 1),
    "F": (2, 0, 136, 1, 7, 17, 3),
    "G": (1, 0, 8, 1, 2, 1, 1),
    "H": (2, 1, 256, 1, 7, 33, 1),
    "I": (2, 0, 128, 1, 6, 16, 1),
    "J": (2, 1, 128, 2, 9, 17, 1),
}


@pytest.mark.parametrize("c", list(R.CASES))
def test_rule_table(c):
    r = R.rules(R.CASES[c])
    got = (r["nsplit"], r["tail_rows"], r["Mg"], r["tail_per"], r["hs_per"], r["w_groups"], r["atom_columns"])
    assert got == EXPECTED[c], (c, r)


def test_what_the_cases_were_chosen_for():
    """The remarks of the case table that the seven rule values do not state."""
    C = R.CASES
    assert sorted(C) == list("ABCDEFGHIJ")
    assert C["A"][1] % R.W_FB == 1                                         # last bin group holds 1 bin
    n, F, N = C["B"]
    assert R.tail_vec4(N) and N - R.ATOMS_PER_WG == 4 and -(-N // R.TN_BN) == 3
    assert -(-n // R.tail_per(n)) == 500 < R.TT_SPLITS                      # ranges 500..511 of 512 hold no frame
    assert [R.split_frames(n, 5, s) for s in range(5)] == [(0, 224), (224, 448), (448, 672), (672, 896), (896, 1000)]
    n, F, N = C["C"]
    assert not R.tail_vec4(N) and N % 4 == 1
    n, F, N = C["D"]
    fr = [R.split_frames(n, 21, s) for s in range(21)]
    assert fr[18] == (4032, 4200) and fr[19] == fr[20] == (4200, 4200)      # two trailing splits are empty
    assert R.tail_per(n) == 8 + 1 and R.hs_per(n) == 8 * 8 + 2 and n - 63 * R.hs_per(n) == 42
    n, F, N = C["E"]
    assert R.tail_rows(F) == R.TN_TAIL_MAX and N % 4 == 2 and N - R.TN_BN == 2
    n, F, N = C["F"]
    assert n % R.TN_BK != 0 and F % 128 == 5 and R.tail_rows(F) == 0 and R.Mg(F) == R.pad4(F) == 136
    assert R.row_regions(F) == (128, 133)
    n, F, N = C["G"]
    assert n < R.OBJ_ROWS and F < R.W_FB and N < 4
    n, F, N = C["I"]
    assert F == 128 and N == R.ATOMS_PER_WG and R.row_regions(F) == (F, F)
    n, F, N = C["J"]
    assert n - 256 * R.tail_per(n) == 1
    # the rule at its own edges
    assert [R.tail_rows(F) for F in (1, 4, 128, 129, 132, 133, 256, 257, 260, 261)] == [0, 0, 0, 1, 4, 0, 0, 1, 4, 0]
    assert [R.nsplit(n, 128, 12) for n in (383, 384, 575, 576, 12287, 12288, 100000)] == [1, 2, 2, 3, 63, 64, 64]
    # where whole rounds of 512 workgroups decide: 516 x 1000 on 32k frames is 40 tiles, 12 splits (the figure
    # csrc/snmf.hip quotes, from before the tail pass took row 512); the 32 tiles of Mg(513) = 512 rows take 16
    assert R.pick_splits(516, 1000, 32768, R.TR_MAX_SPLITS) == 12
    assert R.nsplit(32768, R.Mg(513), 1000) == 16


@pytest.mark.parametrize("c", list(R.CASES))
def test_float32_yardstick_is_a_quarter_of_the_bounds(c):
    """The float32 run of the reference against its float64 run stays within a quarter of every bound, at every run
    of the case that a bound is used on (the slack allows for another BLAS on another host)."""
    for cc, beta, steps, update_w in R.PLAN:
        if cc != c:
            continue
        e = R.yardstick(R.CASES[c], beta, R.MASKS[c], steps, update_w)
        print("%s beta %g steps %d update_w %d: %s" % (c, beta, steps, update_w, R.fmt(e)))
        assert not R.over_bound({k: 4.0 * np.asarray(v) for k, v in e.items()}), (c, beta, steps, update_w, e)


def test_bounds_are_below_one_frame():
    n_max = max(s[0] for s in R.CASES.values())
    assert max(R.W_BOUND, R.H_BOUND, R.OBJ_BOUND) < 1.0 / n_max
    assert R.MODE_TOL + max(R.W_BOUND, R.H_BOUND, R.OBJ_BOUND) < 1.0 / n_max


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_bounds_reject_the_mutant(mutant):
    """Every mutant is at least 4 x the bound away from the unmutated step, in the region that names it, at every
    case where the mistake can show."""
    betas, cases, region = MUTANTS[mutant]
    assert cases
    for c in cases:
        for beta in betas:
            V, W0, H0, ref = _unmutated(c, beta)
            e = R.errors(_one_step(V, W0, H0, R.SPARSITY, beta, R.CASES[c], mutant), ref, R.CASES[c])
            keys = [k for k in e if k == region or (region.endswith(("[rows", ">=")) and k.startswith(region))]
            if region == "W[rows":
                keys = [k for k in keys if "<" not in k]
            assert len(keys) == 1, (region, list(e))
            ratio = float(np.max(e[keys[0]])) / R.bound_of(keys[0])
            print("%s  %s beta %g: %s = %.1f x its bound" % (mutant, c, beta, keys[0], ratio))
            assert ratio >= 4.0, (mutant, c, beta, keys[0], ratio)
