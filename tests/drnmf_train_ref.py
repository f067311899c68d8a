"""fp64 references of the DR-NMF training kernels one stage at a time (csrc/cell_backward.hip, csrc/train.hip), built
on the torch restatement in oracle/drnmf_torch_ref.py (cell_outputs / head_terms: the two halves of model_loss), and
the kernels' selection rules restated in plain Python.  No GPU needed; tests/test_drnmf_train_ref_host.py pins this
file, tests/test_gpu_train_edges.py uses it."""
import numpy as np
import torch

from oracle import drnmf_torch_ref as TR
# ONE restatement of gemm_tn::pick_splits / work_of for both edge suites
from test_gpu_lstm_train_edges import pick_splits, empty_splits           # noqa: F401  (re-exported)


def _t(v, dtype=torch.float64):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().to(dtype)
    return torch.as_tensor(np.asarray(v, dtype=np.float64)).to(dtype)


# ---- the stages -----------------------------------------------------------------------------------------------

def cell_vjp(x, alt, labels_per_k, K, log_h0, cot, mask_value=-1.0, initial_state=None, divergence='ed', beta=1.5,
             dtype=torch.float64):
    """The BPTT alone, the contract of drnmf_cell_backward* for ANY d_out: torch.autograd.grad of the last layer's
    outputs [B,T,N] with grad_outputs=cot, w.r.t. every alt tensor and log_h0.  Returns {name: gradient, ...,
    'log_h0': gradient} as fp64 numpy arrays; a tensor autograd reports as unused (log_h0 with an entering state,
    log_U1 of the KL cell, everything when no frame is valid) comes back as zeros.  dtype=torch.float32: the same
    graph in the device's arithmetic precision, the yardstick for a slice that needs more than G_TOL."""
    leaves = {k: _t(v, dtype).clone().requires_grad_(True) for k, v in alt.items()}
    lh0 = _t(log_h0, dtype).clone().requires_grad_(True)
    init = None if initial_state is None else _t(initial_state, dtype)
    hs = TR.cell_outputs(_t(x, dtype), leaves, labels_per_k, K, lh0, mask_value, divergence, beta, init)
    names = list(leaves) + ['log_h0']
    ts = list(leaves.values()) + [lh0]
    if not hs.requires_grad:
        gs = [None] * len(ts)
    else:
        gs = torch.autograd.grad(hs, ts, grad_outputs=_t(cot, dtype), allow_unused=True)
    return {n: (np.zeros(tuple(t.shape)) if g is None else g.double().numpy()) for n, t, g in zip(names, ts, gs)}


def _head(x_raw, hidden, kc, kn, y, w, square, l1_weight):
    hidden, kc, kn = (_t(v).clone().requires_grad_(True) for v in (hidden, kc, kn))
    x_raw, w = _t(x_raw), _t(w)
    y = x_raw if y is None else _t(y)
    sse, cnt, _ = TR.head_terms(x_raw, y, w, hidden, kc, kn, square, l1_weight)
    sse.backward()
    return float(sse.detach()), float(cnt), hidden.grad.numpy(), kc.grad.numpy(), kn.grad.numpy()


def head_loss_and_grads(x_raw, hidden, kc, kn, y, w, square=False):
    """The mask head alone, the contract of drnmf_loss_head_backward for ANY hidden [rows, 2r]: per row
    w * mean_F (x_raw * mask - y)^2.  Returns (sum, #rows with w != 0, d_hidden, d_kc, d_kn), unnormalised."""
    return _head(x_raw, hidden, kc, kn, y, w, square, None)


def snmf_cost_head_grads(x_raw, hidden, kc, kn, w, l1_weight):
    """The pretraining head alone (drnmf_snmf_cost_head_backward): per row w * (0.5 mean_F (A + Bn - x_raw)^2 +
    l1_weight mean_n |h|).  Same returns."""
    return _head(x_raw, hidden, kc, kn, None, w, False, l1_weight)


def head_forward_ref(hidden, kc, kn, square=False):
    """(mask, A, Bn) of the head in fp64 (A, Bn after the optional squaring: what the device's head hands on)."""
    hidden, kc, kn = _t(hidden), _t(kc), _t(kn)
    r = hidden.shape[-1] // 2
    A, Bn = hidden[..., :r] @ torch.exp(kc), hidden[..., r:] @ torch.exp(kn)
    if square:
        A, Bn = A * A, Bn * Bn
    mask = torch.exp(torch.log(TR.EPS + A) - torch.log(TR.EPS + A + Bn))
    return mask.numpy(), A.numpy(), Bn.numpy()


def relu_margin(x, alt, labels_per_k, K, log_h0, rows=None, mask_value=-1.0, initial_state=None, divergence='ed',
                beta=1.5):
    """How far the fp64 run stays from the kink of the ReLU: the smallest |pre-activation| over valid frames, layers
    and atoms of the batch rows `rows` (all when None), divided by max|h| of those frames (inf without a valid
    frame).  An activation within fp32 rounding of 0 may take the other side on the device, where its derivative
    differs by 1: a case with a max-based bound asserts this margin first.  It depends on the reference alone."""
    x = _t(x)
    pre = []
    with torch.no_grad():
        TR.cell_outputs(x, {k: _t(v) for k, v in alt.items()}, labels_per_k, K, _t(log_h0), mask_value, divergence,
                        beta, None if initial_state is None else _t(initial_state), pre_acts=pre)
    valid = (x != mask_value).any(-1)
    sel = torch.zeros(x.shape[0], dtype=torch.bool)
    sel[list(range(x.shape[0])) if rows is None else list(rows)] = True
    best, hmax = float('inf'), 0.0
    for t, k, p in pre:
        m = valid[:, t] & sel
        if m.any():
            best = min(best, float(p[m].abs().min()))
            hmax = max(hmax, float(p[m].max()))
    if best == float('inf'):
        return best
    return best / max(hmax, 1e-300)


# ---- the selection rules, restated ----------------------------------------------------------------------------
# As pick_splits in tests/test_gpu_lstm_train_edges.py: these mirrors CANNOT SEE THE HEADERS.  They exist so that a
# case named after a branch fails its precondition when the rule it was computed with is no longer the one written
# here -- whoever changes a rule in csrc/ changes it here and re-derives the cases.

ROWS, ATOMS, MAX_TAIL = 16, 32, 2
TN_SPLITS = 64                  # cell_backward.hip TN_SPLITS, train.hip HB_SPLITS
CR_SPLITS = 256
GRAM_MAX_WORK = 3000000


def _rup(v, m):
    return (v + m - 1) // m * m


def tn_plan(M, N, rows):
    """(splits, empty splits) of a time-batched weight-gradient product gemm_tn(M x N over `rows`)."""
    s = pick_splits(M, N, rows, TN_SPLITS)
    return s, empty_splits(rows, s)


def odd_bin(F, divergence='ed'):
    """cell_backward_impl `odd`: F = 16 j + 1 -- the GEMMs run M = F - 1 rows and the last bin's row of d log_D
    comes from S1 / S2 of the column reduction."""
    return F % 16 == 1 and F > 16 and divergence == 'ed'


def bptt_gemm_m(F, divergence='ed'):
    return F - 1 if odd_bin(F, divergence) else _rup(F, 16)


def cr_split_rows(sp, BT):
    """cr_split_rows: the frames [r0, r1) that split sp of the column reduction sums (r0 >= r1: none)."""
    per = (BT + CR_SPLITS - 1) // CR_SPLITS
    return sp * per, min(sp * per + per, BT)


def cr_split_of(bt, BT):
    return bt // ((BT + CR_SPLITS - 1) // CR_SPLITS)


def colreduce_form(N):
    """launch_colreduce: the <V, LANES, U> instance."""
    if N % 4 == 0 and N // 4 <= 64:
        return (4, 4, 4)
    return (4, 1, 4) if N % 4 == 0 else (1, 1, 8)


def fold_form(N):
    """launch_colreduce_fold: split lanes of colreduce_fold_kernel."""
    return 4 if N <= 512 else 1


def dlogd_form(F, N):
    """('scalar', 0, 0) = dlogd_kernel, or ('vec', bins per thread, bin groups) = dlogd_sum / dlogd_apply."""
    if N % 4:
        return ('scalar', 0, 0)
    bpt = 1 if ((N // 4 + 63) // 64) * ((F + 15) // 16) < 128 else 4
    return ('vec', bpt, (F + 4 * bpt - 1) // (4 * bpt))


def ntail_of(F, divergence='ed'):
    return F % 16 if (divergence == 'ed' and F % 16 != 0 and F % 16 <= MAX_TAIL and F > 16) else 0


def nft_main_of(F, divergence='ed'):
    return F // 16 if ntail_of(F, divergence) else _rup(F, 16) // 16


def gram_of(B, N, K, env=None, divergence='ed'):
    """gram_eligible + gram_wanted of an fp32 cell (env = the value of DRNMF_GRAM, or None)."""
    Np = _rup(N, 32)
    if divergence != 'ed' or K < 2 or N > 4096:
        return False
    if Np * Np > GRAM_MAX_WORK:
        return env == 1
    if env in (0, 1):
        return env == 1
    return (_rup(B, ROWS) // ROWS) * Np * Np <= GRAM_MAX_WORK


def rb_of(B, F, N, env=None, gram=False):
    """Workspace.RB of a whole (unsplit) fp32 call; env = DRNMF_RB."""
    groups = _rup(B, 2 * ROWS) // (2 * ROWS)
    numA = _rup(N, 32) // ATOMS
    rb = 2 if (groups * numA >= 500 and groups * nft_main_of(F) * 2 >= 500) else 1
    if env in (1, 2):
        rb = env
    return 1 if gram else rb


def ks_of(B, F, N, env=None, rb_env=None, divergence='ed'):
    """(KS, nch_ks) of the factored fp32 cell: atom ranges per bin tile and 16-atom chunks per range (env, rb_env =
    the values of DRNMF_KS and DRNMF_RB, or None)."""
    rb = rb_of(B, F, N, rb_env)
    Bp = _rup(B, ROWS * rb)
    tiles = (Bp // (ROWS * rb)) * nft_main_of(F, divergence)
    nchN = _rup(N, 32) // 16
    KS = 1
    while KS < (2 if rb > 1 else 4) and tiles * KS < 192 and nchN // (KS * 2) >= 4:
        KS *= 2
    # (a forced count is taken only if it leaves no range empty: cell_b has no path for a range without chunks)
    if env in (1, 2, 4, 8) and (rb == 1 or env <= 2) and (env - 1) * ((nchN + env - 1) // env) < nchN:
        KS = env
    if divergence != 'ed':
        KS = 1
    return KS, (nchN + KS - 1) // KS


def qred_of(B, F, N, ks_env=None, rb_env=None):
    """qred_wanted: cell_b adds the odd-bin partials (more than 64 atom blocks, enough workgroups for the rows)."""
    KS, _ = ks_of(B, F, N, ks_env, rb_env)
    return ntail_of(F) > 0 and _rup(N, 32) // ATOMS > 64 and nft_main_of(F) * KS >= 16 * rb_of(B, F, N, rb_env)


def frames_per_graph(K, T):
    """cell_backward_impl: frames_per_graph(800, 2 K - 1, T)."""
    return min(max(800 // (2 * K - 1), 1), 64, T)


def head_plan(rows, F, r):
    """(Fp4, blocks of 4 rows, splits of the kernel-gradient product, its empty splits) of the two loss heads."""
    Fp4 = _rup(F, 4)
    s = pick_splits(r, Fp4, rows, TN_SPLITS)
    return Fp4, (rows + 3) // 4, s, empty_splits(rows, s)
