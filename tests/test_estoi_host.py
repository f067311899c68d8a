"""CPU-side tests of ESTOI: the fp64 restatement in estoi_ref.py [ESTOI-memory] against itself, the C ABI of
include/drnmf_estoi.h and its argument validation on an unbound handle (no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import estoi_ref as ER
import stoi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_estoi.h")
NAMES = {"drnmf_stoi_ext_workspace_bytes", "drnmf_stoi_ext"}


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
    assert declared == set(capi.ESTOI_SIGNATURES), declared ^ set(capi.ESTOI_SIGNATURES)
    for other in (capi.SIGNATURES, capi.LSTM_SIGNATURES, capi.SCORE_SIGNATURES, capi.ENHANCE_SIGNATURES,
                  capi.SDR_SIGNATURES, capi.DATASET_SIGNATURES, capi.STREAM_SIGNATURES, capi.SNMF_SIGNATURES,
                  capi.SNMF_F16_SIGNATURES, capi.TARGET_SIGNATURES):
        assert not (declared & set(other))
    # drnmf_stoi plus estoi_out behind stoi_out and d_ext_out behind the envelopes
    base = capi.SCORE_SIGNATURES["drnmf_stoi"]
    assert capi.ESTOI_SIGNATURES["drnmf_stoi_ext"] == \
        (base[0], base[1][:8] + [ctypes.c_void_p] + base[1][8:11] + [ctypes.c_void_p] + base[1][11:])
    assert capi.ESTOI_SIGNATURES["drnmf_stoi_ext_workspace_bytes"] == \
        capi.SCORE_SIGNATURES["drnmf_stoi_workspace_bytes"]
    L = capi.lib()
    for name in sorted(declared):
        fn = getattr(L, name)                 # exported ...
        assert fn.argtypes == capi.ESTOI_SIGNATURES[name][1]         # ... and bound by _capi.lib()
        assert fn.restype == capi.ESTOI_SIGNATURES[name][0]
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "no C compiler"
    c = tmp_path / "estoi_header_check.c"
    c.write_text('#include "drnmf_estoi.h"\ntypedef void (*fn_t)(void);\nstatic const fn_t refs[] = {\n' +
                 "".join("    (fn_t)%s,\n" % n for n in sorted(declared)) +
                 "};\nint main(void) { return refs[0] != 0 ? 0 : 1; }\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(c)], check=True)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in doc, name


def test_workspace_bytes(capi):
    L = capi.lib()
    for fs in (8000, 10000, 16000, 48000):
        for n_sig, n in ((1, 0), (1, 300), (3, 16000), (7, 16000 * 4 + 17)):
            base = L.drnmf_stoi_workspace_bytes(n_sig, n, fs)
            ext = L.drnmf_stoi_ext_workspace_bytes(n_sig, n, fs)
            S = max(L.drnmf_stoi_vad_frames(n, fs) - 30, 1)
            assert base > 0 and ext >= base + n_sig * S * 8, (fs, n_sig, n)
            assert ext % 256 == 0
    for fs in (0, -16000, 44100, 22050, 11025):
        assert L.drnmf_stoi_ext_workspace_bytes(1, 1000, fs) == 0
    assert L.drnmf_stoi_ext_workspace_bytes(0, 1000, 16000) == 0


def test_stoi_ext_validates_without_a_gpu(capi):
    """On a drnmf_create_unbound handle: bad arguments -> DRNMF_ERR_INVALID_ARG, an unsupported fs ->
    DRNMF_ERR_UNSUPPORTED, a short or misaligned workspace -> DRNMF_ERR_WORKSPACE, each with a message; a valid call
    gets as far as the device it does not have (DRNMF_ERR_HIP) without enqueuing anything."""
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)          # never dereferenced: nothing is enqueued on this handle
        lens = (ctypes.c_int64 * 3)(16000, 12000, 9000)
        need = L.drnmf_stoi_ext_workspace_bytes(3, 16000, 16000)
        assert need > L.drnmf_stoi_workspace_bytes(3, 16000, 16000)

        def call(n_sig=3, stride=16000, lengths=lens, fs=16000, est=fake, ref=fake, stoi=fake, estoi=fake, d=None,
                 ws=fake, nb=need, handle=h):
            return L.drnmf_stoi_ext(handle, n_sig, stride, lengths, fs, est, ref, stoi, estoi, None, None, None, d, ws,
                                    nb, None)

        def said(*words):
            msg = L.drnmf_last_error(h)
            return len(msg) > 0 and b"stoi_ext" in msg and all(w in msg for w in words)

        assert call(handle=None) == -1
        assert call(stoi=None, estoi=None) == -1 and said(b"bad argument")          # both outputs NULL ...
        assert call(stoi=None, estoi=None, d=fake) == -1 and said(b"bad argument")  # ... d_ext_out is no score
        for kw in (dict(n_sig=0), dict(n_sig=65536), dict(stride=0), dict(lengths=None), dict(est=None), dict(ref=None),
                   dict(ws=None)):
            assert call(**kw) == -1 and said(b"bad argument"), kw
        assert call(stride=12000) == -1 and said(b"lengths[0]")                    # lengths[0] > stride
        neg = (ctypes.c_int64 * 3)(16000, -1, 9000)
        assert call(lengths=neg) == -1 and said(b"lengths[1]")
        for fs in (44100, 22050, 0, -8000):
            assert call(fs=fs) == -2 and said(b"fs"), fs                           # DRNMF_ERR_UNSUPPORTED
        assert call(nb=need - 1) == -4 and said(b"workspace")                      # DRNMF_ERR_WORKSPACE
        assert call(nb=L.drnmf_stoi_workspace_bytes(3, 16000, 16000)) == -4        # drnmf_stoi's is too small
        assert call(ws=ctypes.c_void_p(0x100080)) == -4 and said(b"aligned")
        need10 = L.drnmf_stoi_ext_workspace_bytes(3, 16000, 10000)
        assert 0 < need10 < need
        assert call(fs=10000, nb=need10 - 1) == -4
        for kw in (dict(), dict(stoi=None), dict(estoi=None), dict(d=fake), dict(fs=10000, nb=need10)):
            assert call(**kw) == -3 and said(b"no device"), kw                     # only the device is missing
    finally:
        L.drnmf_destroy(h)


def test_reference_scores_a_signal_against_itself_as_one():
    rng = np.random.default_rng(0)
    for fs in (10000, 16000):
        x = R.speech_like(rng, fs * 2, fs)
        val, parts = ER.estoi(x, x, fs, return_parts=True)
        assert abs(val - 1.0) < 1e-12
        assert parts["d_ext"].shape == (parts["env_ref"].shape[0] - 29,)
        assert abs(ER.estoi(x, 3.0 * x, fs) - 1.0) < 1e-12       # the row normalisation removes a gain
        assert ER.estoi_from_env(parts["env_ref"], parts["env_est"]) == val


def test_reference_is_nan_below_30_frames():
    rng = np.random.default_rng(1)
    for n in (0, 100, 257, 128 * 30 + 256):                  # <= 29 band frames after compaction
        x = R.speech_like(rng, n, 10000, gaps=False) if n else np.zeros(0)
        val, parts = ER.estoi(x, x, 10000, return_parts=True)
        assert np.isnan(val) and parts["d_ext"].shape == (0,), n
        assert parts["env_ref"].shape[0] <= 29
    x = R.speech_like(rng, 128 * 31 + 256, 10000, gaps=False)
    val, parts = ER.estoi(x, x, 10000, return_parts=True)
    assert parts["env_ref"].shape[0] == 30 and parts["d_ext"].shape == (1,) and abs(val - 1.0) < 1e-12


def test_reference_is_nan_where_stoi_is_not():
    """Plain arithmetic: a silent stretch of the estimate makes whole columns zero, their norm 0 and d = 0/0."""
    fs = 10000
    rng = np.random.default_rng(7)
    x = R.speech_like(rng, fs * 3, fs, gaps=False)
    y = x.copy()
    y[fs:2 * fs] = 0.0
    val, parts = ER.estoi(x, y, fs, return_parts=True)
    assert np.isnan(val) and np.isfinite(parts["stoi"]) and 0.5 < parts["stoi"] < 1.0
    assert np.isnan(parts["d_ext"]).any() and np.isfinite(parts["d_ext"]).any()
    val, parts = ER.estoi(x, np.zeros_like(x), fs, return_parts=True)
    assert np.isnan(val) and np.isnan(parts["d_ext"]).all() and abs(parts["stoi"] - 1.0) < 1e-12
    env = np.abs(rng.standard_normal((40, 15))) + 1.0
    flat = env.copy()
    flat[:, 3] = 2.0                                         # a band constant over every segment: its row norm is 0
    assert np.isfinite(ER.estoi_from_env(env, env)) and np.isnan(ER.estoi_from_env(env, flat))


@pytest.mark.parametrize("fs", [10000, 16000])
def test_estoi_is_not_stoi_on_the_rows_the_gpu_test_scores(fs):
    """The GPU test cannot pass by returning STOI: on the noisy rows the two lie more than 0.05 apart, and ESTOI
    falls as the noise rises."""
    lengths, E, X, want = ER.oracle_batch(fs)
    assert len(lengths) == 6 and min(lengths) >= 1.9 * fs and max(lengths) <= 3.4 * fs
    vals = [v for v, _ in want]
    for i, (val, parts) in enumerate(want):
        assert np.isfinite(val) and parts["env_ref"].shape[0] >= 30
        if i % 5 != 4:                                       # plus noise (row 4 is the low-passed copy)
            assert abs(val - parts["stoi"]) > 0.05, (i, val, parts["stoi"])
    assert vals[0] < vals[1] < vals[2] < vals[3] < vals[4]   # -5, 0, 5, 10 dB, low-passed
    assert 0.05 < min(vals) and max(vals) < 1.0


def test_extended_flags_default_to_off():
    import inspect
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import layers, ops
    assert inspect.signature(ops.stoi).parameters["extended"].default is False
    assert inspect.signature(ops.compute_scores).parameters["extended"].default is False
    assert inspect.signature(layers._SequenceModel.enhance).parameters["extended_scores"].default is False
    assert list(inspect.signature(ops.estoi).parameters)[:3] == ["est", "ref", "fs"]
    assert ops.SCORE_LABELS == ['SDR', 'SNR', 'SegSNR local', 'SegSNR global', 'PESQ', 'STOI']
