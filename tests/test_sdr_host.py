"""CPU-side tests of the device-side SDR: the C ABI of include/drnmf_sdr.h, its argument validation on an unbound
handle, and the argument checks of ops.sdr_db that need no device (no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_sdr.h")
NAMES = {"drnmf_toeplitz_solve", "drnmf_sdr_ragged_workspace_bytes", "drnmf_sdr_ragged"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(drnmf_[a-z0-9_]+)\s*\(", src))


def test_sdr_header_is_plain_c_and_matches_the_binding(capi, tmp_path):
    declared = _declared(HDR)
    assert declared == NAMES
    assert declared == set(capi.SDR_SIGNATURES), declared ^ set(capi.SDR_SIGNATURES)
    for other in (capi.SIGNATURES, capi.LSTM_SIGNATURES, capi.SCORE_SIGNATURES, capi.ENHANCE_SIGNATURES):
        assert not (declared & set(other))
    for hdr in ("drnmf.h", "drnmf_score.h"):
        assert not (_declared(os.path.join(ROOT, "include", hdr)) & NAMES), hdr
    L = capi.lib()
    for name in sorted(declared):
        fn = getattr(L, name)                 # exported ...
        assert fn.argtypes == capi.SDR_SIGNATURES[name][1]       # ... and bound by _capi.lib()
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "no C compiler"
    src = tmp_path / "sdr_header_check.c"
    src.write_text('#include "drnmf_sdr.h"\ntypedef void (*fn_t)(void);\nstatic const fn_t refs[] = {\n' +
                   "".join("    (fn_t)%s,\n" % n for n in sorted(declared)) +
                   "};\nint main(void) { return refs[0] != 0 ? 0 : 1; }\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_workspace_query(capi):
    L = capi.lib()
    q = L.drnmf_sdr_ragged_workspace_bytes
    for shape in ((0, 1000, 512), (3, 0, 512), (3, 1000, 0), (-1, 1000, 512), (3, 1000, 2049)):
        assert q(*shape) == 0, shape
    # r, d, coef in fp64 and the correlation partials of every 8192-sample span at the very least
    assert q(3, 48000, 512) >= 3 * 512 * 8 * 3 + 3 * 6 * 2 * 512 * 8
    assert q(3, 48000, 512) % 256 == 0
    assert q(3, 96000, 512) > q(3, 48000, 512) > q(3, 48000, 32)


def test_entry_points_validate_without_a_gpu(capi):
    """On a drnmf_create_unbound handle every bad argument returns DRNMF_ERR_INVALID_ARG (a short workspace
    DRNMF_ERR_WORKSPACE) with a message, before anything is enqueued."""
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)          # never dereferenced: validation fails first

        def solve(handle=h, n_sys=3, n=512, r=fake, d=fake, c=fake, info=fake):
            return L.drnmf_toeplitz_solve(handle, n_sys, n, r, d, c, info, None)

        assert solve(handle=None) == -1
        for kw in (dict(n_sys=0), dict(n_sys=-2), dict(n=0), dict(n=-1), dict(n=2049)):
            assert solve(**kw) == -1, kw
        assert b"toeplitz_solve" in L.drnmf_last_error(h)
        for kw in (dict(r=None), dict(d=None), dict(c=None), dict(info=None)):
            assert solve(**kw) == -1, kw
        assert b"NULL" in L.drnmf_last_error(h)

        need = L.drnmf_sdr_ragged_workspace_bytes(3, 48000, 512)
        assert need > 0

        def sdr(handle=h, n_sig=3, stride=48000, lengths=fake, flen=512, est=fake, ref=fake, out=fake, ws=fake,
                nb=need):
            return L.drnmf_sdr_ragged(handle, n_sig, stride, lengths, flen, est, ref, out, None, None, None, None,
                                      None, ws, nb, None)

        assert sdr(handle=None) == -1
        for kw in (dict(n_sig=0), dict(n_sig=65536), dict(stride=0), dict(stride=-5), dict(flen=0),
                   dict(flen=2049)):
            assert sdr(**kw) == -1, kw
        assert b"sdr_ragged" in L.drnmf_last_error(h)
        for kw in (dict(est=None), dict(ref=None), dict(out=None), dict(ws=None)):
            assert sdr(**kw) == -1, kw
        assert b"NULL" in L.drnmf_last_error(h)
        assert sdr(nb=need - 1) == -4             # DRNMF_ERR_WORKSPACE
        assert sdr(nb=0) == -4
        assert sdr(lengths=None, nb=need - 1) == -4            # lengths may be NULL: every row at full stride
        assert b"workspace" in L.drnmf_last_error(h)
    finally:
        L.drnmf_destroy(h)


def test_sdr_db_refuses_lengths_on_the_host_solver_and_unknown_solvers(capi):
    import torch
    from drnmf_amd import ops
    e, r = torch.zeros(2, 1000), torch.ones(2, 1000)
    with pytest.raises(ValueError, match="lengths"):
        ops.sdr_db(e, r, lengths=[1000, 500], solver="host")
    with pytest.raises(ValueError, match="lengths"):
        ops.sdr_db(e, r, lengths=[1000, 500])                  # the default solver is the host's
    with pytest.raises(ValueError, match="solver"):
        ops.sdr_db(e, r, solver="lapack")
    with pytest.raises(ValueError, match="sdr_solver"):
        ops.compute_scores(e, r, 16000, sdr_solver="lapack")
