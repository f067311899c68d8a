"""The argument rules of drnmf_amd.ops that every wrapper shares: what a caller-supplied `out`, state or workspace must
be (ops._out, ops._check_state, ops._workspace), and the text a refused entry point raises with (ops._call).

Nothing here checks numbers against a reference: the other GPU suites do.  A case is a handful of launches at
B = 1, T = 2, F = 5, N = 4, K = 2; every refusal happens in Python or in the library's own argument checks, before
any launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, T, F, N, K = 1, 2, 5, 4, 2
ENTRIES = ["cell_forward", "dense_cell_forward", "cell_forward_ista", "snmf_mask_forward", "snmf_kl_forward",
           "snmf_online_forward", "lstm_head_forward"]
STATEFUL = ["cell_forward", "dense_cell_forward", "cell_forward_ista"]
WORKSPACES = ["snmf_mask_workspace", "snmf_adapt_workspace", "snmf_online_workspace", "mix_workspace"]


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    return ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


@pytest.fixture(scope="module")
def entries(ops):
    """name -> (call(out=None, **states) -> the entry's result, out's shape).  Inputs are made once."""
    rng = np.random.RandomState(3)
    r = lambda *s: _t(rng.rand(*s) + 0.05)
    x, log_h0 = r(B, T, F), _t(np.log(rng.rand(N) + 0.05))
    e = {}

    desc = ops.make_desc(B, T, F, N, K)
    logs = (_t(np.log(rng.rand(1, F, N) + 0.05)), _t(np.zeros((1, 1))), _t(np.full(1, np.log(0.1))))
    params = ops.prepare_params(desc, *logs)
    e["cell_forward"] = (lambda out=None, **st: ops.cell_forward(x, -1.0, params, desc, log_h0, (1.0, 0.0, 0.0),
                                                                  out=out, **st), (B, T, N))
    desc_kl = ops.make_desc(B, T, F, N, K, divergence="kl")
    params_kl = ops.prepare_params(desc_kl, *logs)
    e["cell_forward_ista"] = (lambda out=None, **st: ops.cell_forward_ista(x, -1.0, params_kl, desc_kl, log_h0,
                                                                            out=out, **st), (B, T, N))
    ddesc = ops.make_dense_desc(B, T, F, N, K)
    dparams = ops.dense_prepare_params(ddesc, 0.1 * r(K, N, N), 0.1 * r(K - 1, N, N), 0.1 * r(K, F, N), 0.1 * r(K, N))
    h0 = r(N)
    e["dense_cell_forward"] = (lambda out=None, **st: ops.dense_cell_forward(x, -1.0, dparams, ddesc, h0, out=out,
                                                                              **st), (B, T, N))
    W = rng.rand(F, N) + 0.05
    nrm = np.sqrt((W * W).sum(0))
    Wn, h_init = _t(W / nrm), _t(rng.rand(N) * nrm)
    e["snmf_mask_forward"] = (lambda out=None: ops.snmf_mask_forward(x, Wn, h_init, 0.1, 3, mask_value=-1.0, out=out),
                              (B, T, F))
    e["snmf_kl_forward"] = (lambda out=None: ops.snmf_kl_forward(x, Wn, h_init, 0.1, 3, mask_value=-1.0, out=out),
                            (B, T, F))
    state = ops.snmf_online_state(B, F, N, N // 2, 16, Wn, DEV)

    def online(out=None):
        ops.snmf_online_reset(state, Wn)
        return ops.snmf_online_forward(x, h_init, 0.1, 3, N // 2, state, mask_value=-1.0, out=out)
    e["snmf_online_forward"] = (online, (B, T, F))

    H = N
    ldesc = ops.make_lstm_desc(B, T, F, H, K)
    w = lambda *s: _t(rng.standard_normal(s) * 0.3)
    lparams = ops.lstm_prepare_params(ldesc, [w(F, 4 * H), w(H, 4 * H)], [w(H, 4 * H), w(H, 4 * H)],
                                      [w(4 * H), w(4 * H)], w(H, F), w(F))
    hidden = w(B, T, H)
    e["lstm_head_forward"] = (lambda out=None: ops.lstm_head_forward(hidden, lparams, ldesc, out=out), (B, T, F))
    return e


def _noncontiguous(shape, device=DEV):
    """A float32 view of `shape` that is not contiguous: transposed, or (where a dimension of 1 makes the transpose
    contiguous again) every other element of a wider last dimension."""
    t = torch.zeros(shape[::-1], dtype=torch.float32, device=device).permute(*range(len(shape) - 1, -1, -1))
    if t.is_contiguous():
        t = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=torch.float32, device=device)[..., ::2]
    assert tuple(t.shape) == tuple(shape) and not t.is_contiguous()
    return t


def _other_device():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second device")
    return "cuda:1"


@pytest.mark.parametrize("name", ENTRIES)
def test_a_correct_out_is_used_and_changes_nothing(entries, name):
    call, shape = entries[name]
    want = call()
    assert tuple(want.shape) == shape and want.dtype == torch.float32 and want.is_contiguous()
    out = torch.full(shape, 7.0, dtype=torch.float32, device=DEV)
    got = call(out=out)
    assert got is out
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("name", ENTRIES)
def test_a_wrong_out_is_refused(entries, name):
    call, shape = entries[name]
    with pytest.raises(ValueError, match="out must be a contiguous torch.float32 tensor"):
        call(out=torch.zeros(shape, dtype=torch.float16, device=DEV))
    with pytest.raises(ValueError, match="out must be a contiguous torch.float32 tensor"):
        call(out=_noncontiguous(shape))


@pytest.mark.parametrize("name", ENTRIES)
def test_an_out_on_another_device_is_refused(entries, name):
    call, shape = entries[name]
    with pytest.raises(ValueError, match="out must be a contiguous torch.float32 tensor"):
        call(out=torch.zeros(shape, dtype=torch.float32, device=_other_device()))


@pytest.mark.parametrize("which", ["initial_state", "final_state"])
@pytest.mark.parametrize("name", STATEFUL)
def test_a_wrong_state_is_refused(entries, name, which):
    call = entries[name][0]
    good = torch.zeros((B, N), dtype=torch.float32, device=DEV)
    assert call(**{which: good}) is not None
    for bad in (torch.zeros((B, N), dtype=torch.float16, device=DEV), _noncontiguous((B, N))):
        with pytest.raises(ValueError, match="%s must be a contiguous torch.float32 tensor" % which):
            call(**{which: bad})


@pytest.mark.parametrize("which", ["initial_state", "final_state"])
@pytest.mark.parametrize("name", STATEFUL)
def test_a_state_on_another_device_is_refused(entries, name, which):
    with pytest.raises(ValueError, match="%s must be a contiguous torch.float32 tensor" % which):
        entries[name][0](**{which: torch.zeros((B, N), dtype=torch.float32, device=_other_device())})


def _workspace_call(ops, name):
    """(fn(have) -> workspace, the bytes the library asks for) of one of the four public workspace helpers."""
    L = ops._capi.lib()
    if name == "snmf_mask_workspace":
        return (lambda have: ops.snmf_mask_workspace("gemm", B, T, F, N, 2.0, DEV, have=have),
                L.drnmf_snmf_mask_workspace_bytes(B, T, F, N))
    if name == "snmf_adapt_workspace":
        return (lambda have: ops.snmf_adapt_workspace(B, T, F, N, N // 2, DEV, have=have),
                L.drnmf_snmf_adapt_workspace_bytes(B, T, F, N, N // 2))
    if name == "snmf_online_workspace":
        return (lambda have: ops.snmf_online_workspace(B, T, F, N, N // 2, 16, DEV, have=have),
                L.drnmf_snmf_online_workspace_bytes(B, T, F, N, N // 2, 16))
    return lambda have: ops.mix_workspace(3, 100, DEV, have=have), L.drnmf_mix_workspace_bytes(3, 100)


@pytest.mark.parametrize("name", WORKSPACES)
def test_workspace_reuse(ops, name):
    fn, need = _workspace_call(ops, name)
    assert need > 1
    fresh = fn(None)
    assert fresh.dtype == torch.uint8 and fresh.numel() == need and fresh.device == torch.device(DEV)
    short = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    got = fn(short)
    assert got is not short and got.dtype == torch.uint8 and got.numel() == need
    exact = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert fn(exact) is exact
    larger = torch.empty(need + 3, dtype=torch.uint8, device=DEV)
    assert fn(larger) is larger
    floats = torch.empty(need, dtype=torch.float32, device=DEV)          # 4 * need bytes, but not uint8
    got = fn(floats)
    assert got is not floats and got.dtype == torch.uint8 and got.numel() == need


def test_workspace_on_another_device_is_replaced(ops):
    other = _other_device()
    for name in WORKSPACES:
        fn, need = _workspace_call(ops, name)
        got = fn(torch.empty(need, dtype=torch.uint8, device=other))
        assert got.device == torch.device(DEV) and got.numel() == need


def test_the_tile_path_needs_no_workspace(ops):
    assert ops.snmf_mask_path("tile", B * T, F, N) == "tile"
    assert ops.snmf_mask_workspace("tile", B, T, F, N, 2.0, DEV) is None
    assert ops.snmf_mask_workspace("tile", B, T, F, N, 2.0, DEV, have=torch.empty(8, dtype=torch.uint8,
                                                                                 device=DEV)) is None


def test_a_refused_entry_names_itself(ops):
    """ops._call's text: "<entry> failed (<code>): <the library's message>"."""
    rng = np.random.RandomState(5)
    x, Wn, hn = _t(rng.rand(B, T, F)), _t(rng.rand(F, N)), _t(rng.rand(N))
    # n_fixed = N + 1: the sizing refuses it first, in Python, as it did before the entries shared one call
    with pytest.raises(ValueError, match=r"^snmf_adapt: shape B=1 T=2 F=5 N=4 n_fixed=5 is not taken"):
        ops.snmf_adapt_forward(x, Wn, hn, 0.1, 3, N + 1)
    # the library's own refusal, through _call: a workspace one byte long, which drnmf_dense_cell_forward compares
    # with its layout before it enqueues anything (DRNMF_ERR_WORKSPACE = -4, include/drnmf.h)
    desc = ops.make_dense_desc(B, T, F, N, K)
    params = ops.dense_prepare_params(desc, _t(np.zeros((K, N, N))), _t(np.zeros((K - 1, N, N))),
                                      _t(np.zeros((K, F, N))), _t(np.zeros((K, N))))
    with pytest.raises(ValueError, match=r"^drnmf_dense_cell_forward failed \(-4\): dense_cell_forward: workspace"):
        ops.dense_cell_forward(x, None, params, desc, hn, workspace=torch.empty(1, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    ops.check_status(DEV)
