"""The resampler's reference (tests/resample_ref.py) against scipy and against itself, and what the library answers
without a GPU: the ABI's symbols and binding, the rate reduction, the size queries and the refusals."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_resample.h")
NAMES = {"drnmf_resample_rate", "drnmf_resample_taps_len", "drnmf_resample_out_len", "drnmf_resample_tile",
         "drnmf_resample_taps", "drnmf_resample_forward", "drnmf_resample_chunk", "drnmf_resample_carry"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


def _noise(n, seed):
    return np.random.RandomState(seed).standard_normal(n)


@pytest.mark.parametrize("fs_in,fs_out,p,q", R.RATE_PAIRS)
def test_reference_equals_scipy_resample_poly(fs_in, fs_out, p, q):
    sig = pytest.importorskip("scipy.signal")
    assert R.rate(fs_in, fs_out) == (p, q)
    if p == q:
        return
    h = R.filter_taps(p, q)
    for n in (1, 2, 777, 3001):
        x = _noise(n, 10 * p + q + n)
        want = sig.resample_poly(x, p, q, window=h / p, padtype='constant')
        got = R.resample(x, p, q, h)
        assert got.shape == want.shape == (R.out_len(n, p, q),)
        assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("fs_in,fs_out,p,q", R.RATE_PAIRS)
def test_chunked_reference_equals_the_offline_one_exactly(fs_in, fs_out, p, q):
    h = np.ones(1) if p == q else R.filter_taps(p, q)
    L = len(h)
    for n in (0, 1, 333):
        x = _noise(n, n + p).astype(np.float32)
        want = R.resample(x, p, q, None if p == q else h)
        for name, cuts in R.chunkings(n, seed=n + q, big=100).items():
            hist = []
            got = R.resample_chunked(x, p, q, cuts, history=hist)
            assert got.shape == want.shape and np.array_equal(got, want), (n, name)
            # the history a later push needs: at most about (L - 1) / p + q / p + 1 samples
            assert max(hist) <= (L - 1) // p + q // p + 2, (n, name, max(hist))


def test_rate_reduction_and_output_lengths(capi):
    from drnmf_amd import ops
    for fs_in, fs_out, p, q in R.RATE_PAIRS + ((44100, 48000, 160, 147), (48000, 44100, 147, 160), (16000, 8000, 1, 2),
                                               (16000, 11025, 441, 640), (16000.0, 48000, 3, 1)):
        assert ops.resample_rate(fs_in, fs_out) == (p, q)
        lens = np.array([0, 1, 2, 3, 441, 16000, 64000, 2 ** 33 + 5], dtype=np.int64)
        want = np.array([-(-int(n) * p // q) for n in lens], dtype=np.int64)
        got = ops.resample_out_lengths(lens, fs_in, fs_out)
        assert got.dtype == np.int64 and np.array_equal(got, want)
        for n, w in zip(lens, want):
            assert capi.lib().drnmf_resample_out_len(int(n), p, q) == w
            assert R.out_len(n, p, q) == w


def test_refusals(capi):
    from drnmf_amd import ops
    L = capi.lib()
    p, q = ctypes.c_int32(-7), ctypes.c_int32(-7)
    for fs_in, fs_out in ((0, 16000), (16000, 0), (-8000, 16000), (16000, -1), (16000, 44101), (44101, 16000),
                          (16000, 16000 * 641)):
        with pytest.raises(ValueError):
            ops.resample_rate(fs_in, fs_out)
        with pytest.raises(ValueError):
            ops.resample_out_lengths([5], fs_in, fs_out)
        with pytest.raises(ValueError):
            R.rate(fs_in, fs_out)
        assert L.drnmf_resample_rate(fs_in, fs_out, ctypes.byref(p), ctypes.byref(q)) == -1
        assert (p.value, q.value) == (-7, -7)
    for bad in (16000.5, float("nan"), float("inf"), None, "16000", True):
        with pytest.raises(ValueError):
            ops.resample_rate(bad, 16000)
    with pytest.raises(ValueError):
        ops.resample_out_lengths([3, -1], 48000, 16000)
    with pytest.raises(ValueError):
        ops.resample_tile(48000, 16000, nz=0)
    with pytest.raises(ValueError):
        ops.resample_tile(11025, 16000, nz=16)        # 2 * 16 * 640 + 1 taps of fp64 do not fit in 160 KiB


def test_size_queries(capi):
    L = capi.lib()
    for p, q, nz in ((0, 1, 10), (1, 0, 10), (-1, 3, 10), (641, 1, 10), (1, 641, 10), (1, 3, 0), (1, 3, -1),
                     (640, 441, 16), (1, 640, 16)):
        assert L.drnmf_resample_taps_len(p, q, nz) == 0, (p, q, nz)
        assert L.drnmf_resample_tile(p, q, nz) == 0, (p, q, nz)
    for n, p, q in ((-1, 1, 3), (5, 0, 3), (5, 1, 0), (5, 641, 1), (2 ** 40 + 1, 1, 3)):
        assert L.drnmf_resample_out_len(n, p, q) == 0, (n, p, q)
    assert L.drnmf_resample_taps_len(1, 1, 10) == 0 and L.drnmf_resample_tile(1, 1, 10) == capi.RESAMPLE_TILE
    lds = 160 * 1024
    for p in range(1, 641):
        for q in (1, 2, 3, 7, 160, 441, 639, 640):
            taps, tile = L.drnmf_resample_taps_len(p, q, 10), L.drnmf_resample_tile(p, q, 10)
            if p == q == 1:
                continue
            assert taps == 2 * 10 * max(p, q) + 1 and 1 <= tile <= capi.RESAMPLE_TILE, (p, q, taps, tile)
            # the table and the samples a tile's outputs can meet fit in the LDS of a compute unit
            span = (q * (tile - 1) + taps - 1) // p + 1
            assert 8 * taps + 4 * (span + 1) <= lds, (p, q, taps, tile)
            if tile < capi.RESAMPLE_TILE:               # and one output more would not
                assert 8 * taps + 4 * ((q * tile + taps - 1) // p + 2) > lds, (p, q, taps, tile)
    for p, q in ((1, 3), (2, 1), (160, 441), (441, 160), (640, 441), (147, 160), (1, 6)):
        assert L.drnmf_resample_tile(p, q, 10) == capi.RESAMPLE_TILE, (p, q)
    assert L.drnmf_resample_tile(1, 640, 10) == 4


def test_equal_rates_filter_is_a_unit_impulse():
    """p == q (here the unreduced 3 / 3 and 160 / 160): at the sample instants the taps are a unit impulse, so the
    definition's sum is the sample itself -- what the copy path returns without a filter."""
    for p in (1, 3, 160):
        h = R.filter_taps(p, p)
        half = (len(h) - 1) // 2
        at = h[half % p::p]
        want = np.zeros_like(at)
        want[half // p] = at[half // p]
        assert np.abs(at - want).max() <= 1e-15 * abs(at[half // p])
    x = _noise(500, 3).astype(np.float32)
    assert np.array_equal(R.resample(x, 1, 1), x.astype(np.float64))
    i16 = (x * 3000).astype(np.int16)
    assert np.array_equal(R.resample(i16, 1, 1).astype(np.float32), i16.astype(np.float32) / np.float32(32768.0))


def test_reference_tones():
    """No quality claim beyond the definition: a 1 kHz tone survives 48 -> 16 kHz, a 12 kHz tone does not."""
    h = R.filter_taps(1, 3)
    t = np.arange(48000 // 4) / 48000.0
    mid = slice(200, -200)
    y1 = R.resample(np.sin(2 * np.pi * 1000 * t), 1, 3, h)
    want = np.sin(2 * np.pi * 1000 * np.arange(y1.shape[0]) / 16000.0)
    assert np.abs(y1 - want)[mid].max() <= 1e-3
    y12 = R.resample(np.sin(2 * np.pi * 12000 * t), 1, 3, h)
    assert 3.5e-4 <= np.abs(y12)[mid].max() < 4.5e-4         # 4e-4 to one digit (4.06e-4): -68 dB, folded to 4 kHz


@pytest.mark.parametrize("fs_in,fs_out,p,q", R.RATE_PAIRS)
def test_rounded_reference_stays_within_one_float32_rounding(fs_in, fs_out, p, q):
    x = _noise(1500, p + q).astype(np.float32)
    y = R.resample(x, p, q)
    assert np.abs(y.astype(np.float32).astype(np.float64) - y).max() <= 2.0 ** -24 * np.abs(y).max()


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return set(re.findall(r"\b(drnmf_[a-z0-9_]+)\s*\(", src))


def test_resample_header_is_plain_c_and_matches_the_binding(capi, tmp_path):
    declared = _declared()
    assert declared == NAMES
    assert declared == set(capi.RESAMPLE_SIGNATURES), declared ^ set(capi.RESAMPLE_SIGNATURES)
    for t in dir(capi):
        if t.endswith("SIGNATURES") and t != "RESAMPLE_SIGNATURES":
            assert not (declared & set(getattr(capi, t))), t
    L = capi.lib()
    for name in sorted(declared):
        fn = getattr(L, name)                 # exported ...
        assert fn.argtypes == capi.RESAMPLE_SIGNATURES[name][1]       # ... and bound by _capi.lib()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in declared:
        assert name in doc, name
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "no C compiler"
    src = tmp_path / "resample_header_check.c"
    src.write_text('#include "drnmf_resample.h"\ntypedef void (*fn_t)(void);\nstatic const fn_t refs[] = {\n' +
                   "".join("    (fn_t)%s,\n" % n for n in sorted(declared)) +
                   "};\nint main(void) { return refs[0] != 0 && DRNMF_RESAMPLE_MAX_PQ == %d && DRNMF_RESAMPLE_TILE == %d"
                   " && DRNMF_RESAMPLE_NZ == %d && DRNMF_RESAMPLE_BETA == %r ? 0 : 1; }\n"
                   % (capi.RESAMPLE_MAX_PQ, capi.RESAMPLE_TILE, capi.RESAMPLE_NZ, capi.RESAMPLE_BETA))
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_resample_entry_points_validate_without_a_gpu(capi):
    """On a drnmf_create_unbound handle: every bad shape, rate and required NULL pointer returns
    DRNMF_ERR_INVALID_ARG with a message, and a fully valid call stops only at the missing device."""
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)          # never dereferenced: the call stops before any launch

        def forward(handle=h, n_sig=3, si=1001, ln=fake, i16=1, x=fake, p=1, q=3, nz=10, taps=fake, so=335, y=fake):
            return L.drnmf_resample_forward(handle, n_sig, si, ln, i16, x, p, q, nz, taps, so, y, None)

        def chunk(handle=h, n_sig=3, si=1001, ln=fake, a=fake, b=fake, c=fake, d=fake, i16=0, x=fake, p=160, q=441,
                  nz=10, taps=fake, so=335, y=fake):
            return L.drnmf_resample_chunk(handle, n_sig, si, ln, a, b, c, d, i16, x, p, q, nz, taps, so, y, None)

        def carry(handle=h, n_sig=3, i16=0, sp=100, prev=fake, sc=50, ch=fake, drop=fake, keep=fake, add=fake, sn=150,
                  nxt=fake):
            return L.drnmf_resample_carry(handle, n_sig, i16, sp, prev, sc, ch, drop, keep, add, sn, nxt, None)

        def taps(handle=h, p=160, q=441, nz=10, beta=5.0, out=fake):
            return L.drnmf_resample_taps(handle, p, q, nz, beta, out, None)

        rates = (dict(p=0), dict(q=0), dict(p=641), dict(q=641), dict(p=2, q=6), dict(nz=0), dict(p=640, q=441, nz=16))
        for call, who, bad, pointers, optional in (
                (forward, b"resample_forward",
                 (dict(n_sig=0), dict(n_sig=-2), dict(si=0), dict(si=-7), dict(so=0), dict(so=-1), dict(i16=2),
                  dict(i16=-1)) + rates, ("ln", "x", "taps", "y"), ()),
                (chunk, b"resample_chunk",
                 (dict(n_sig=0), dict(si=0), dict(so=0), dict(i16=2)) + rates, ("ln", "x", "taps", "y"),
                 ("a", "b", "c", "d")),
                (carry, b"resample_carry",
                 (dict(n_sig=0), dict(n_sig=65536), dict(i16=2), dict(sp=0), dict(sc=-1), dict(sn=0)),
                 ("prev", "ch", "drop", "keep", "add", "nxt"), ()),
                (taps, b"resample_taps",
                 rates + (dict(p=1, q=1), dict(beta=-1.0), dict(beta=float("nan")), dict(beta=float("inf"))),
                 ("out",), ())):
            assert call(handle=None) == -1
            for kw in bad:
                assert call(**kw) == -1, (who, kw)
                assert who in L.drnmf_last_error(h), (kw, L.drnmf_last_error(h))
            for name in pointers:
                assert call(**{name: None}) == -1, (who, name)
                assert who in L.drnmf_last_error(h) and b"NULL" in L.drnmf_last_error(h)
            for kw in [dict()] + [{name: None} for name in optional]:
                rc = call(**kw)
                assert rc not in (0, -1, -2, -4) and who in L.drnmf_last_error(h) and \
                    b"no device" in L.drnmf_last_error(h), (who, kw, rc)
        # the copy needs no filter, and nothing to add needs no chunk
        for rc in (forward(p=1, q=1, taps=None), carry(sc=0, ch=None)):
            assert rc not in (0, -1, -2, -4) and b"no device" in L.drnmf_last_error(h)
    finally:
        L.drnmf_destroy(h)
