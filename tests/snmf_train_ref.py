"""The reference, the case table and the bounds of the sparse-NMF dictionary-training kernels (csrc/snmf.hip:
drnmf_snmf_train_init / drnmf_snmf_train_step), and the kernels' selection rules restated in plain Python.  numpy
only, no GPU needed; tests/test_snmf_train_ref_host.py pins this file, tests/test_gpu_snmf_train_edges.py uses it.

Layout: the oracle's (sparse_nmf_gpu.m's) -- V (F, n), W (F, N), H (N, n).  The device holds the transposes of V and H
(frames are rows there); the GPU test transposes at the boundary.
"""
import numpy as np

from oracle import drnmf_oracle as O


# ---- the reference --------------------------------------------------------------------------------------------

def step_reference(V, W0, H0, sparsity, steps, beta, w_ind, update_w=True, dtype=np.float64):
    """`steps` iterations of oracle.sparse_nmf_train from explicit inits, in `dtype` (the oracle computes in V's type).
    w_ind: None (every atom is updated) or a bool mask of the atoms to update; update_w=False switches the W update
    off whatever the mask says (the oracle skips it when no entry is true).  Returns W, H, div[steps], cost[steps]."""
    N = np.shape(W0)[1]
    if not update_w:
        w_ind = np.zeros(N, bool)
    W, H, obj = O.sparse_nmf_train(np.asarray(V, dtype=dtype), np.asarray(W0, dtype=dtype),
                                   np.asarray(H0, dtype=dtype), float(sparsity), int(steps), 0.0, beta, w_ind)
    return W, H, np.asarray(obj["div"]), np.asarray(obj["cost"])


# ---- the selection rules, restated ----------------------------------------------------------------------------
# These mirrors CANNOT SEE csrc/.  They exist so that a case named after a branch fails its expectation
# (tests/test_snmf_train_ref_host.py holds the values as literals) when the rule it was chosen with is no longer the
# one written here -- whoever changes a rule in csrc/ changes it here and re-derives the cases.

TR_MAX_SPLITS = 64              # snmf.hip
TN_BM = TN_BN = 128             # gemm_tn.h: output tile
TN_BK = 32                      # gemm_tn.h: contraction rows per k-tile
TN_MIN_STEPS = 192              # gemm_tn::pick_splits: contraction steps every split keeps
TN_TAIL_MAX, TT_SPLITS = 4, 512
HS_SPLITS = 64
W_FB = 8                        # bins per workgroup row of w_fold / w_apply / w_norm
ATOMS_PER_WG = 256              # threads (atoms) per workgroup column of the thread-per-atom kernels
OBJ_ROWS = 128                  # gemm_nt.h BM: frames per partial of the fused objective sums


def _cdiv(a, b):
    return (a + b - 1) // b


def pad4(F):
    return _cdiv(F, 4) * 4


def pick_splits(M, N, Kdim, max_splits):
    """gemm_tn::pick_splits."""
    tiles = _cdiv(M, TN_BM) * _cdiv(N, TN_BN)
    best, best_cost = 1, 1e30
    for s in range(1, max_splits + 1):
        if s > 1 and Kdim // s < TN_MIN_STEPS:
            break
        cost = float((tiles * s + 511) // 512) / s * (1.0 + 0.004 * s)
        if cost < best_cost - 1e-9:
            best_cost, best = cost, s
    return best


def tail_rows(F):
    """tn_tail_rows: the 1..TN_TAIL_MAX bins behind whole 128-row tiles that the streaming tail pass takes."""
    return F % 128 if (F > 128 and 1 <= F % 128 <= TN_TAIL_MAX) else 0


def Mg(F):
    """Rows of the two TN products: F without its tail rows, or F padded to a multiple of 4."""
    return F - tail_rows(F) if tail_rows(F) else pad4(F)


def nsplit(n, Mg_, N):
    """tr_splits: the split-K count of NUM = V'^T H and DEN = P1^T H."""
    return pick_splits(Mg_, N, n, TR_MAX_SPLITS)


def split_frames(n, ns, s):
    """gemm_tn work_of: the frames [r0, r1) that split s of ns contracts (r0 >= r1: an empty split)."""
    nkt = _cdiv(n, TN_BK)
    per = _cdiv(nkt, ns)
    return min(s * per * TN_BK, n), min((s + 1) * per * TN_BK, n)


def tail_per(n):
    """Frames per row range of tn_tail_kernel."""
    return _cdiv(n, TT_SPLITS)


def hs_per(n):
    """Frames per row range of colsum_rows_kernel (the beta == 1 W update's column sums of H)."""
    return _cdiv(n, HS_SPLITS)


def w_groups(F):
    return _cdiv(F, W_FB)


def atom_columns(N):
    return _cdiv(N, ATOMS_PER_WG)


def tail_vec4(N):
    """tn_tail_kernel<true> (four atoms per thread) or <false>."""
    return N % 4 == 0


def rules(case):
    """Every rule value of a case, in the order the GPU test prints and the host test pins them."""
    n, F, N = case
    return dict(nsplit=nsplit(n, Mg(F), N), tail_rows=tail_rows(F), Mg=Mg(F), tail_per=tail_per(n),
                hs_per=hs_per(n), w_groups=w_groups(F), atom_columns=atom_columns(N))


def row_regions(F):
    """(first row, end) of W's rows apart from the whole row tiles of the TN products: the tail rows, or the rows of
    a padded last tile (F % 128 >= 5); (F, F) when there are none."""
    if F > 128 and F % 128:
        return F - F % 128, F
    return F, F


# ---- the cases ------------------------------------------------------------------------------------------------
# (n frames, F bins, N atoms): each the smallest shape that reaches its branch
CASES = {
    "A": (300, 65, 12),       # the existing anchor: nsplit 1, no tail, last bin group holds 1 bin
    "B": (1000, 130, 260),    # nsplit 5 (a full group of four + one clamped), 2 tail rows <true>, tail_per 2 (ranges
                              # 500..511 hold no frame), 4 atoms in a second workgroup column, 3 TN column tiles
    "C": (1000, 131, 37),     # 3 tail rows, odd N: tn_tail_kernel<false>, scalar GEMM instances, no rider column
    "D": (4200, 129, 12),     # nsplit 21 (two of them empty), tail_per 9: the 8-frame loop twice, 7 clamped slots;
                              # hs_per 66 = 8 unrolled rounds + 2, last range short (42)
    "E": (800, 132, 130),     # nsplit exactly 4, 4 tail rows = TN_TAIL_MAX, N % 4 == 2, second column tile 2 wide
    "F": (389, 133, 516),     # nsplit 2 with n % 32 != 0, F % 128 = 5: no tail pass, Mg = Fp4 = 136, 3 wg columns
    "G": (100, 7, 3),         # everything below one tile, F below one bin group, n below one row tile
    "H": (385, 257, 200),     # two row tiles + 1 tail row, nsplit 2: the shipped model's shape in small
    "I": (384, 128, 256),     # the control without edges
    "J": (513, 129, 4),       # tail_per 2 with the last non-empty range holding one frame
}
SPARSITY = 0.1
GEN_RANK = 12                 # rank of the non-negative factors V is generated from (the parity test's)


def w_ind(N, kind):
    """None | 'thirds' (every third atom frozen, atom 0 included) | 'none' (all false) -> None or a bool mask."""
    if kind is None:
        return None
    if kind == "thirds":
        return np.arange(N) % 3 != 0
    if kind == "none":
        return np.zeros(N, bool)
    raise ValueError(kind)


def problem(case, beta, seed=8):
    """float32 V (F, n), W0 (F, N), H0 (N, n) as tests/test_gpu_parity.test_snmf_training_matches_oracle builds them:
    a low-rank non-negative V plus 1e-3, un-normalised W0 in [0, 2), H0 in [0, 1); for beta != 2, 1 % of V is exactly
    0 so that the min-positive floor runs."""
    n, F, N = case
    rng = np.random.default_rng(seed)
    r = min(N, GEN_RANK)
    Wt = rng.random((F, r))
    V = (Wt @ (rng.random((r, n)) * (rng.random((r, n)) < 0.4)) + 1e-3).astype(np.float32)
    if beta != 2.0:
        V[rng.random(V.shape) < 0.01] = 0.0
    W0 = rng.random((F, N)).astype(np.float32) * 2
    H0 = rng.random((N, n)).astype(np.float32)
    return V, W0, H0


# ---- errors and bounds ----------------------------------------------------------------------------------------

def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def errors(got, ref, case):
    """got, ref: (W, H, div[], cost[]).  Relative max errors max|d| / max|ref| of H, of W as a whole and of W's regions,
    each region normalised by its own reference maximum (absent regions are left out); |d| / |ref| of div and cost per
    step.  Keys name the region: they are what a failing assertion prints."""
    n, F, N = case
    Wg, Hg, dg, cg = got
    Wr, Hr, dr, cr = ref
    Wg, Wr = np.asarray(Wg, np.float64), np.asarray(Wr, np.float64)
    r0, r1 = row_regions(F)
    e = {"H": _rel(Hg, Hr), "W": _rel(Wg, Wr)}
    main = min(r0, F)
    e["W[rows < %d: whole row tiles]" % main] = _rel(Wg[:main], Wr[:main])
    if r0 < r1:
        what = "tail rows" if tail_rows(F) else "padded last tile"
        e["W[rows %d..%d: %s]" % (r0, r1 - 1, what)] = _rel(Wg[r0:r1], Wr[r0:r1])
    e["W[atoms < %d]" % ATOMS_PER_WG] = _rel(Wg[:, :ATOMS_PER_WG], Wr[:, :ATOMS_PER_WG])
    if N > ATOMS_PER_WG:
        e["W[atoms >= %d]" % ATOMS_PER_WG] = _rel(Wg[:, ATOMS_PER_WG:], Wr[:, ATOMS_PER_WG:])
    dr, cr = np.asarray(dr, np.float64), np.asarray(cr, np.float64)
    e["div"] = np.abs(np.asarray(dg, np.float64) - dr) / np.abs(dr)
    e["cost"] = np.abs(np.asarray(cg, np.float64) - cr) / np.abs(cr)
    return e


def yardstick(case, beta, kind, steps=3, update_w=True, seed=8):
    """errors() of the float32 run of step_reference against its float64 run on the same inputs."""
    V, W0, H0 = problem(case, beta, seed)
    m = w_ind(case[2], kind)
    ref = step_reference(V, W0, H0, SPARSITY, steps, beta, m, update_w)
    f32 = step_reference(V, W0, H0, SPARSITY, steps, beta, m, update_w, dtype=np.float32)
    return errors(f32, ref, case)


# Bounds = 8 x the largest float32 yardstick (above) over the cases and betas that use the bound, rounded up to one
# significant digit.  The device adds the same fp32 terms in other orders and through more partials than numpy does
# (up to 21 split-K partials, 512 tail ranges, 64 column-sum ranges), each reordering worth about the fp32 error
# itself; and 8 keeps every bound below 1/n for the largest n used (2.4e-4 at n = 4200): one dropped or doubled
# frame of a frame sum does not fit.  None of them comes from device output (DESIGN.md lists the device errors).
# The yardsticks are the maxima over PLAN below (every case, its betas, 1 and 3 steps, and the three-step H-only runs
# of A..D), measured with numpy on the build host's CPU; the host test holds each of them to a quarter of its bound.
YARDSTICK_FACTOR = 8
W_BOUND = 9e-6                  # yardstick 1.07e-6 (F, beta 2, 3 steps), every region of W
H_BOUND = 2e-5                  # yardstick 1.58e-6 (B, beta 1, 3 H-only steps)
OBJ_BOUND = 3e-6                # yardstick 3.16e-7 (C, beta 1.5, 3 steps); beta 1 and 2 alone: 2.79e-7 (D, beta 2, H-only)
#                                 -- within a factor of 3 of each other, so div and cost share one constant at every beta
UNIT_NORM_TOL = 1e-5            # the project's existing bar on W's column norms (tests/test_gpu_parity.py)
MODE_TOL = 5e-5                 # the project's existing mode-to-mode bar (tests/test_gpu_x3.py)


def bound_of(key, beta=None):
    if key == "H":
        return H_BOUND
    if key.startswith("W"):
        return W_BOUND
    return OBJ_BOUND


def over_bound(errs, widen=0.0):
    """[(region, error, bound)] of every entry of errors() above its bound (+ widen): empty when all is well."""
    bad = []
    for k, v in errs.items():
        b = bound_of(k) + widen
        if not float(np.max(v)) <= b:
            bad.append((k, float(np.max(v)), b))
    return bad


def fmt(errs):
    return "  ".join("%s %.2e" % (k, float(np.max(v))) for k, v in errs.items())


# what the GPU test runs: the mask per case, the betas per case (1.5 / 0: the P2 / P1 numerator-denominator pair with
# floored zeros, on B and C only), and the H-only cases
MASKS = {c: (None if c in "ADGIJ" else "thirds") for c in CASES}
H_ONLY = ("A", "B", "C", "D")


def betas_of(c):
    return (2.0, 1.0, 1.5, 0.0) if c in "BC" else (2.0, 1.0)


# (case, beta, steps, update_w) of every run a bound is used on
PLAN = [(c, b, s, True) for c in CASES for b in betas_of(c) for s in (1, 3)] + \
       [(c, b, 3, False) for c in H_ONLY for b in (2.0, 1.0)]
