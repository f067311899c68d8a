"""CPU-side tests of the sparse-NMF baseline on fp16 operands: the C ABI of include/drnmf_snmf_f16.h (exports,
binding, admission rule, argument validation on an unbound handle), the operand_dtype argument of
layers.SparseNMFModel / build_snmf, and the fp64 emulation of tests/snmf_f16_ref.py the GPU tests lean on: its
distance from the fp64 oracle and the algebra of the per-row scale (no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import snmf_f16_ref as E
import snmf_model_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_snmf_f16.h")
NAMES = {"drnmf_snmf_f16_admitted", "drnmf_snmf_f16_dict_bytes", "drnmf_snmf_f16_pack_dict", "drnmf_snmf_f16_forward"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


def test_header_is_plain_c_and_matches_the_binding(capi, tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(drnmf_[a-z0-9_]+)\s*\(", src))
    assert declared == NAMES
    assert declared == set(capi.SNMF_F16_SIGNATURES), declared ^ set(capi.SNMF_F16_SIGNATURES)
    for other in (capi.SIGNATURES, capi.LSTM_SIGNATURES, capi.SCORE_SIGNATURES, capi.ENHANCE_SIGNATURES,
                  capi.SDR_SIGNATURES, capi.DATASET_SIGNATURES, capi.STREAM_SIGNATURES, capi.SNMF_SIGNATURES):
        assert not (declared & set(other))
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(HDR).read()) == ["drnmf.h"]
    L = capi.lib()
    for name in sorted(declared):
        fn = getattr(L, name)                 # exported ...
        assert fn.argtypes == capi.SNMF_F16_SIGNATURES[name][1]      # ... and bound by _capi.lib()
        assert fn.restype == capi.SNMF_F16_SIGNATURES[name][0]
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "no C compiler"
    c = tmp_path / "snmf_f16_header_check.c"
    c.write_text('#include "drnmf_snmf_f16.h"\ntypedef void (*fn_t)(void);\nstatic const fn_t refs[] = {\n' +
                 "".join("    (fn_t)%s,\n" % n for n in sorted(declared)) +
                 "};\nint main(void) { return refs[0] != 0 ? 0 : 1; }\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(c)], check=True)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in doc, name


def test_admission_rule_and_dictionary_size(capi):
    L = capi.lib()
    adm = L.drnmf_snmf_f16_admitted
    assert adm(257, 512, 2.0) == 1 and adm(257, 200, 2.0) == 1 and adm(5, 10, 2.0) == 1 and adm(1, 2, 2.0) == 1
    assert adm(257, 514, 2.0) == 0 and adm(257, 200, 1.0) == 0 and adm(257, 200, 1.5) == 0
    assert adm(257, 201, 2.0) == 0 and adm(257, 0, 2.0) == 0 and adm(0, 200, 2.0) == 0
    assert capi.SNMF_F16_MAX_N == 512
    q = L.drnmf_snmf_f16_dict_bytes
    assert q(0, 200) == 0 and q(257, 0) == 0
    assert q(257, 200) == 257 * 224 * 2 and q(5, 10) == 5 * 32 * 2 and q(257, 512) == 257 * 512 * 2


def test_entries_validate_before_they_touch_a_device(capi):
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = ctypes.c_void_p(base)
    odd = ctypes.c_void_p(base + 4)

    def fwd(B=1, T=1, F=5, N=10, n_iter=3, sparsity=0.1, power=1.0, has_mask=1, x=p, d16=p, Wn=p, h0=p, out=p):
        return L.drnmf_snmf_f16_forward(h, B, T, F, N, n_iter, sparsity, power, -1.0, has_mask, x, d16, Wn, h0, out,
                                        None)

    def pack(F=5, N=10, Wn=p, d16=p, nbytes=5 * 32 * 2):
        return L.drnmf_snmf_f16_pack_dict(h, F, N, Wn, d16, nbytes, None)
    try:
        assert L.drnmf_snmf_f16_forward(None, 1, 1, 5, 10, 3, 0.1, 1.0, -1.0, 1, p, p, p, p, p, None) == -1
        for bad in (dict(N=11), dict(B=0), dict(T=0), dict(F=0), dict(N=0), dict(n_iter=-1), dict(sparsity=-1.0),
                    dict(sparsity=float("nan")), dict(has_mask=2), dict(x=None), dict(d16=None), dict(Wn=None),
                    dict(h0=None), dict(out=None), dict(d16=odd), dict(Wn=odd), dict(B=1 << 16, T=1 << 16)):
            assert fwd(**bad) == -1, bad
            assert L.drnmf_last_error(h)
        assert fwd(N=514) == -2 and b"514" in L.drnmf_last_error(h)         # DRNMF_ERR_UNSUPPORTED
        assert fwd() == -3 and fwd(N=512) == -3 and fwd(n_iter=0) == -3     # valid: only the device is missing
        assert L.drnmf_snmf_f16_pack_dict(None, 5, 10, p, p, 320, None) == -1
        for bad in (dict(F=0), dict(N=0), dict(Wn=None), dict(d16=None), dict(d16=odd)):
            assert pack(**bad) == -1, bad
        assert pack(nbytes=5 * 32 * 2 - 1) == -4                            # DRNMF_ERR_WORKSPACE
        assert pack() == -3
    finally:
        L.drnmf_destroy(h)


def test_model_arguments_and_the_builder_key(capi):
    from drnmf_amd import layers
    _, W, h_init = R.problem(3, 7, 129, 200)
    mk = lambda **kw: layers.SparseNMFModel(**dict(dict(W=W, r=100, sparsity=0.1, device="cpu"), **kw))
    assert mk().operand_dtype == "float32"                         # the default changes nothing
    m = mk(operand_dtype="float16", path="tile", h_init=h_init)
    assert m.operand_dtype == "float16" and m.path == "tile" and m._stateful() and not m._carries_state()
    assert [w.shape for w in m.get_weights()] == [(129, 200)] and m.get_weights()[0].dtype == np.float32
    with pytest.raises(ValueError, match="operand_dtype"):
        mk(operand_dtype="bfloat16")
    with pytest.raises(ValueError, match="float16"):
        mk(operand_dtype="float16", beta=1.0)
    with pytest.raises(ValueError, match="float16"):
        mk(operand_dtype="float16", path="gemm")
    _, W514, _ = R.problem(*R.WIDE)
    with pytest.raises(ValueError, match="float16"):
        layers.SparseNMFModel(W514, 257, 0.1, operand_dtype="float16", device="cpu")
    assert layers.SparseNMFModel(W514, 257, 0.1, device="cpu").operand_dtype == "float32"
    p = dict(r=100, sparsity=1., cf="ed", random_seed=2016., max_iter=1000., conv_eps=1e-4, display=0.)
    assert layers.build_snmf(p, W, device="cpu").operand_dtype == "float32"
    b = layers.build_snmf(dict(p, operand_dtype="float16"), W, device="cpu")
    assert (b.operand_dtype, b.r, b.n_iter, b.beta, b.path) == ("float16", 100, 200, 2.0, "auto")
    with pytest.raises(ValueError, match="float16"):
        layers.build_snmf(dict(p, cf="kl", operand_dtype="float16"), W, device="cpu")
    from drnmf_amd import ops
    import torch
    x, Wt, ht = torch.zeros(1, 3, 129), torch.from_numpy(W), torch.from_numpy(h_init)
    d16 = torch.zeros(129, 224, dtype=torch.float16)
    with pytest.raises(ValueError, match="shape"):
        ops.snmf_f16_forward(x, d16, Wt[:-1], ht, 0.1, 3)
    with pytest.raises(ValueError, match="even"):
        ops.snmf_f16_forward(x, d16, Wt[:, :199], ht[:199], 0.1, 3)
    with pytest.raises(ValueError, match="dict16"):
        ops.snmf_f16_forward(x, d16[:, :200], Wt, ht, 0.1, 3)
    with pytest.raises(ValueError, match="dict16"):
        ops.snmf_f16_forward(x, d16.float(), Wt, ht, 0.1, 3)


def test_row_scale():
    v = np.array([0.0, 1.0, 0.75, 0.5, 0.5000001, 3.0, 65536.0, 65537.0, 1e-5, np.inf, 1e-45, 1e-13, 3e38], np.float32)
    s = E.row_scale(v)
    assert list(s[:8]) == [1.0, 1.0, 1.0, 2.0, 1.0, 0.25, 2.0 ** -16, 2.0 ** -17]
    assert s[8] == 2.0 ** 16 and s[9] == 1.0                               # 1e-5 in (2^-17, 2^-16]
    assert s[10] == 2.0 ** 40 and s[11] == 2.0 ** 40 and s[12] == 2.0 ** -100      # the exponent is clamped ...
    assert float(np.float16(s.max() * 1e-9)) < 65504                       # ... so the scaled floor is finite in fp16
    ok = np.isfinite(v) & (v >= 2.0 ** -40) & (v <= 2.0 ** 100)
    assert np.all((v[ok] * s[ok] > 0.5) & (v[ok] * s[ok] <= 1.0))


def test_emulation_against_the_oracle():
    """The fp16 operands are visible: on the live case (snmf_f16_ref.LIVE at LIVE_ITER iterations) the emulation is
    at least 4 x TOL_EMU from the fp64 oracle, while the scaled iteration WITHOUT the roundings stays within 1e-6 of
    it; and nowhere is the emulation further than 1e-2 -- masks lie in [0, 1]."""
    for case in E.CASES:
        ref, emu = E.case_reference(*case), E.case_emulation(*case)
        d = float(np.max(np.abs(emu - ref)))
        print("snmf f16 emulation %s: max |emulation - oracle| %.3e" % (case, d))
        assert np.isfinite(emu).all() and emu.min() >= 0 and emu.max() <= 1
        masked = ~E.valid_frames(*case)
        assert not emu[masked].any() and not ref[masked].any()
        assert masked.any() or case[0] * case[1] == 1          # masked rows wherever there is room for one
        assert d <= 1e-2, (case, d)
    x, W, h_init = E.problem(*E.LIVE)
    Wn, hn = R.normalised(W, h_init)
    ref = E.case_reference(*E.LIVE, n_iter=E.LIVE_ITER)
    plain = E.emulate_mask(x, Wn, hn, R.SPARSITY, E.LIVE_ITER, round_operands=False)
    d_plain = float(np.max(np.abs(plain - ref)))
    d_live = float(np.max(np.abs(E.case_emulation(*E.LIVE, n_iter=E.LIVE_ITER) - ref)))
    print("snmf f16 live case %s, %d iterations: rounded %.3e, unrounded %.3e; 4 x TOL_EMU = %.3e" %
          (E.LIVE, E.LIVE_ITER, d_live, d_plain, E.LIVE_MIN_DISTANCE))
    assert d_plain <= 1e-6           # float32 Wn / h_init against the oracle's fp64 normalisation, nothing else
    assert d_live >= E.LIVE_MIN_DISTANCE, d_live


@pytest.mark.parametrize("k", [-3, 5, 14])
def test_emulation_is_unchanged_by_a_power_of_two(k):
    """V, sparsity and h_init times 2^k: the row's scale absorbs the factor and every rounded operand is the same
    number.  What is left are the two terms that are NOT homogeneous, the floor and the 1e-9 of the mask's denominator:
    constants of the problem, so in the scaled iteration they are 1e-9 s and 1e-9 s 2^-k.  The floor binds nowhere
    on these frames; the 1e-9 moves the mask by at most 1e-9 max(s, s 2^-k) / min(Wc Hc + Wn Hn), and the scaled
    reconstruction stays above 1e-4 s (bins of x are at least 1e-3, the reconstruction a tenth of that): 1e-5
    max(1, 2^-k)."""
    B, T, F, N = 1, 17, 33, 48
    x, W, h_init = R.problem(B, T, F, N)
    Wn, hn = R.normalised(W, h_init)
    base = E.emulate_mask(x, Wn, hn, R.SPARSITY, R.N_ITER)
    f = np.float32(2.0 ** k)
    xs = np.where(x == np.float32(R.MASK_VALUE), x, x * f).astype(np.float32)
    got = E.emulate_mask(xs, Wn, hn * f, R.SPARSITY * float(f), R.N_ITER)
    d = float(np.max(np.abs(got - base)))
    print("snmf f16 emulation x 2^%d: max difference %.3e" % (k, d))
    assert d <= 1e-5 * max(1.0, 2.0 ** -k)
    # ... and it is the matching factor on h_init that does it: with h_init left alone two iterations differ
    other = E.emulate_mask(xs, Wn, hn, R.SPARSITY * float(f), 2)
    assert float(np.max(np.abs(other - E.emulate_mask(x, Wn, hn, R.SPARSITY, 2)))) > 1e-4


def test_very_quiet_rows_stay_finite_with_and_without_padding_bins():
    """Rows far below the floor (x 1e-16, x 1e-30: the scale's exponent is clamped at 2^40, the scaled floor is 1100)
    next to ordinary ones: finite, within TOL_EXACT of the oracle, and the same with zero bins appended to x and Wn
    as the kernel's last chunk has them -- no operand is inf, so a zero bin contributes an exact zero."""
    x, W, h_init = E.range_problem()
    Wn, hn = R.normalised(W, h_init)
    emu, ref = E.range_references()
    assert np.isfinite(emu).all()
    for i in (1, 6, 7):
        assert x[0, i].max() > 0 and float(np.max(np.abs(emu[0, i] - ref[0, i]))) <= E.TOL_EXACT, i
    F = x.shape[2]
    pad = 31
    valid = np.any(x != np.float32(R.MASK_VALUE), axis=-1)
    xp = np.concatenate([x, np.where(valid[..., None], np.float32(0), np.float32(R.MASK_VALUE))
                         * np.ones((1, 1, pad), np.float32)], axis=2)
    Wp = np.concatenate([Wn, np.zeros((pad, Wn.shape[1]), np.float32)], axis=0)
    padded = E.emulate_mask(xp, Wp, hn, R.SPARSITY, R.N_ITER)
    assert np.isfinite(padded).all()
    assert np.array_equal(padded[..., :F], emu)


@pytest.mark.parametrize("k", E.SCALED_K)
def test_scaled_problems_need_the_row_scale(k):
    """The live problem times 2^k with sparsity and h_init scaled along: with the per-row scale the emulation is as
    close to the oracle as at k = 0; with every scale forced to 1 it is NOT within TOL_EXACT -- so the GPU test on
    these problems fails for a kernel that drops the scale."""
    emu, ref = E.scaled_references(k)
    d = float(np.max(np.abs(emu - ref)))
    bare, _ = E.scaled_references(k, row_scaled=False)
    with np.errstate(invalid="ignore"):
        d_bare = float(np.nanmax(np.abs(bare - ref))) if np.isfinite(bare).any() else np.inf
    bad = (~np.isfinite(bare)).any()
    print("snmf f16 emulation x 2^%d: with the scale %.3e from the oracle, without %.3e%s" %
          (k, d, d_bare, " and not finite" if bad else ""))
    assert d <= E.TOL_EXACT
    assert bad or d_bare > E.TOL_EXACT
