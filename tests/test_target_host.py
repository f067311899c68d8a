"""CPU-side tests of the training targets: the C ABI of include/drnmf_target.h (export, binding, argument
validation on an unbound handle), the checks ops.wavs_to_tensors / fit_wavs make on `target` before they touch a
device, and the fp64 reference of tests/psa_ref.py against itself (no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import psa_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_target.h")
NAMES = {"drnmf_stft_pair_chunks_target"}


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
    assert declared == set(capi.TARGET_SIGNATURES), declared ^ set(capi.TARGET_SIGNATURES)
    for other in (capi.SIGNATURES, capi.LSTM_SIGNATURES, capi.SCORE_SIGNATURES, capi.ENHANCE_SIGNATURES,
                  capi.SDR_SIGNATURES, capi.DATASET_SIGNATURES, capi.STREAM_SIGNATURES, capi.SNMF_SIGNATURES,
                  capi.SNMF_F16_SIGNATURES):
        assert not (declared & set(other))
    assert capi.TARGETS == {"mag": 0, "psa": 1, "tpsa": 2}
    # drnmf_stft_pair_chunks plus one int32 behind `transform`
    base = capi.DATASET_SIGNATURES["drnmf_stft_pair_chunks"]
    assert capi.TARGET_SIGNATURES["drnmf_stft_pair_chunks_target"] == \
        (base[0], base[1][:13] + [ctypes.c_int32] + base[1][13:])
    L = capi.lib()
    for name in sorted(declared):
        fn = getattr(L, name)                 # exported ...
        assert fn.argtypes == capi.TARGET_SIGNATURES[name][1]        # ... and bound by _capi.lib()
        assert fn.restype == capi.TARGET_SIGNATURES[name][0]
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "no C compiler"
    c = tmp_path / "target_header_check.c"
    c.write_text('#include "drnmf_target.h"\ntypedef void (*fn_t)(void);\nstatic const fn_t refs[] = {\n' +
                 "".join("    (fn_t)%s,\n" % n for n in sorted(declared)) +
                 "};\nint main(void) { return refs[0] != 0 && DRNMF_TARGET_MAG == 0 && DRNMF_TARGET_PSA == 1 &&\n"
                 "                    DRNMF_TARGET_TPSA == 2 ? 0 : 1; }\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(c)], check=True)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in doc, name


def test_entry_point_validates_without_a_gpu(capi):
    """On a drnmf_create_unbound handle: an unknown target and a phase-sensitive target with 'logmag' return
    DRNMF_ERR_INVALID_ARG with a message, every check of drnmf_stft_pair_chunks still holds, and a valid call
    gets as far as the device it does not have (DRNMF_ERR_HIP) without enqueuing anything."""
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)          # never dereferenced: nothing is enqueued on this handle

        def call(handle=h, n_sig=3, sx=1001, sy=999, lx=fake, ly=fake, n_seq=5, table=fake, T=7, N=512, hop=128,
                 i16=1, tr=0, tg=1, px=fake, py=fake, x=fake, y=fake, w=fake):
            return L.drnmf_stft_pair_chunks_target(handle, n_sig, sx, sy, lx, ly, n_seq, table, T, N, hop, i16, tr,
                                                   tg, -1.0, px, py, x, y, w, None)

        who = b"stft_pair_chunks_target"
        assert call(handle=None) == -1
        for tg in (-1, 3, 7):
            assert call(tg=tg) == -1, tg
            assert who in L.drnmf_last_error(h) and b"target" in L.drnmf_last_error(h)
        for tg in (1, 2):
            assert call(tr=1, tg=tg) == -1, tg
            assert who in L.drnmf_last_error(h) and b"TRANSFORM_MAG only" in L.drnmf_last_error(h)
        for kw in (dict(n_sig=0), dict(sx=0), dict(n_seq=0), dict(T=-7), dict(hop=0), dict(i16=2)):
            assert call(**kw) == -1, kw
            assert who in L.drnmf_last_error(h) and b"bad shape" in L.drnmf_last_error(h), kw
        assert call(N=500) == -1 and b"power of two" in L.drnmf_last_error(h)
        assert call(tr=2) == -1 and b"transform" in L.drnmf_last_error(h)
        for name in ("lx", "ly", "table", "px", "py", "x", "y", "w"):
            assert call(**{name: None}) == -1, name
            assert who in L.drnmf_last_error(h) and b"NULL" in L.drnmf_last_error(h)
        for kw in (dict(tg=0), dict(tg=1), dict(tg=2), dict(tg=0, tr=1), dict(N=128, hop=64), dict(N=4096, i16=0)):
            assert call(**kw) == -3, kw                               # DRNMF_ERR_HIP: only the device is missing
            assert who in L.drnmf_last_error(h) and b"no device" in L.drnmf_last_error(h)
    finally:
        L.drnmf_destroy(h)


def test_targets_are_refused_before_the_device_is_touched(capi):
    """These run on a machine without a GPU: the checks come before the first allocation."""
    from drnmf_amd import layers, ops
    a = np.zeros(1000, np.int16)
    with pytest.raises(ValueError, match="target must be"):
        ops.wavs_to_tensors([a], [a], target="irm")
    for target in P.TARGETS:
        with pytest.raises(ValueError, match="transform 'mag' only"):
            ops.wavs_to_tensors([a], [a], transform="logmag", target=target)
    with pytest.raises(TypeError):
        ops.wavs_to_frames([a], [a], 512, 128, target="tpsa")        # the packed frames take no target

    class Fake(layers._SequenceModel):
        mask_value = -1.0

        def __init__(self):
            pass

        def _device(self):
            return "cuda:0"

        def _input_width(self):
            return 257

    with pytest.raises(ValueError, match="target must be"):
        Fake().fit_wavs([a], [a], target="irm")
    with pytest.raises(ValueError, match="transform 'mag' only"):
        Fake().fit_wavs([a], [a], transform="logmag", target="psa")


def _spectra(seed, shape=(33, 40)):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def test_reference_against_itself():
    S, X = _spectra(1), _spectra(2)
    X[:, 7] = 0                                                       # a frame in which the noisy member is silent
    p = P.target("psa", S, X)
    assert p.dtype == np.float64 and np.array_equal(p, P.project(S, X))
    assert np.all(p[:, 7] == 0) and np.all(np.isfinite(p))
    assert np.any(p < 0) and np.any(p > np.abs(X))                    # 'psa' leaves [0, x] on both sides
    live = np.abs(X) > 0
    assert np.allclose(p[live], (np.abs(S) * np.cos(np.angle(S) - np.angle(X)))[live], rtol=0, atol=1e-12)
    assert np.array_equal(p, P.project(np.conj(S), np.conj(X)))      # the stored spectra are conjugated: no matter
    t = P.target("tpsa", S, X)
    assert np.array_equal(t, np.clip(p, 0.0, P.magnitude(X)))        # 'tpsa' = 'psa' clipped
    assert np.all(t >= 0) and np.all(t <= P.magnitude(X)) and np.all(t[:, 7] == 0)
    # a magnitude given from outside (the device's float32 one) is the one divided by and clipped to
    m = np.abs(X).astype(np.float32)
    live = m > 0
    assert np.all(np.abs(P.project(S, X, m) * m - (S * np.conj(X)).real)[live] <= 1e-14 * (np.abs(S) * np.abs(X))[live])
    assert np.all(P.target("tpsa", S, X, m) <= m.astype(np.float64))


def test_reference_on_equal_and_negated_members():
    X = _spectra(3)
    m = np.abs(X)
    for S, want, clipped in ((X, m, m), (-X, -m, np.zeros_like(m))):
        p = P.target("psa", S, X)
        assert np.all(np.abs(p - want) <= 2 * np.spacing(m))          # p = +-m_x within 2 ulp
        assert np.all(np.abs(P.target("tpsa", S, X) - clipped) <= 2 * np.spacing(m))
    assert np.array_equal(P.target("tpsa", -X, X), np.zeros_like(m))  # clean = -noisy: exactly 0


@pytest.mark.parametrize("N,hop", P.R.PAIR_SIZES, ids=P.R.ids(P.R.PAIR_SIZES))
def test_the_pairs_hold_what_the_gpu_tests_need(N, hop):
    for int16 in (True, False):
        kinds, noisy, clean, X64, S64 = P.pairs(N, hop, int16)
        assert len(kinds) == 6 and set(kinds) == {"noise", "longer", "early", "zeros", "same", "negated"}
        lens = [len(c) for c in clean]
        assert min(lens) < N and any(n % hop == 0 for n in lens)
        for kind, x, c, X, S in zip(kinds, noisy, clean, X64, S64):
            assert x.dtype == c.dtype == (np.int16 if int16 else np.float32)
            assert X.shape == S.shape == (N // 2 + 1, P.R.frames(len(c), N, hop))
            # the bound of the independent GPU check is far below the values it checks
            assert np.max(np.abs((S * np.conj(X)).real)) > 1000 * 4 * P.R.TOL_FWD * np.max(np.abs(S)) * np.max(np.abs(X))
            if kind == "longer":
                assert len(x) > len(c)
            elif kind == "early":
                assert len(x) < len(c) and P.R.frames(len(x), N, hop) == P.R.frames(len(c), N, hop)
            elif kind == "zeros":
                zero = np.flatnonzero(np.abs(X).max(axis=0) == 0)
                assert np.any(np.abs(S[:, zero]).max(axis=0) > 0)    # whole frames with m_x == 0 under a live clean one
            elif kind == "same":
                assert np.array_equal(X, S)
            elif kind == "negated":
                assert np.array_equal(X, -S)
