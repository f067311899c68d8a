"""CPU-side tests of STOI (score_audio.m:231): the fp64 restatement in stoi_ref.py [STOI-memory], the C ABI of
include/drnmf_score.h and its argument validation (no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import stoi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_score.h")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


def test_band_table():
    assert R.BANDS == [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55),
                       (55, 69), (69, 87), (87, 109), (109, 138), (138, 174), (174, 219)]
    assert all(hi > lo for lo, hi in R.BANDS)                # none is empty: all 15 survive the rank trim


def test_resample_filter_at_16k():
    h, p, q, half = R.resample_filter(16000)
    assert (p, q) == (5, 8) and len(h) == 161 and half == 80
    assert abs(h[80] - 0.6254) < 5e-5
    assert abs(h.sum() - 5.0) < 1e-12
    assert np.array_equal(h, h[::-1]) or float(np.abs(h - h[::-1]).max()) < 1e-15
    for fs, pq in ((8000, (5, 4)), (32000, (5, 16)), (48000, (5, 24)), (10000, (1, 1))):
        assert R.rate(fs) == pq


@pytest.mark.parametrize("fs", [8000, 16000, 48000])
def test_resampler_equals_upfirdn(fs):
    """Matlab resample = upfirdn with the same taps, the output shifted by the filter delay."""
    signal = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(3).standard_normal(1237)
    h, p, q, half = R.resample_filter(fs)
    ny = -(-len(x) * p // q)
    full = signal.upfirdn(h, x, p, q)
    # y[m] = sum_k x[k] h[q m + half - p k] = full[m + half / q] when q divides half; in general shift the
    # upsampled grid by prepending zeros so that q m + half lands on the grid
    pre = (q - half % q) % q
    full = signal.upfirdn(np.concatenate([np.zeros(pre), h]), x, p, q)
    off = (half + pre) // q
    np.testing.assert_allclose(R.resample(x, fs), full[off:off + ny], rtol=0, atol=1e-12)


def test_stoi_of_itself_and_of_a_scaled_copy():
    rng = np.random.default_rng(0)
    x = R.speech_like(rng, 16000 * 2, 16000)
    assert abs(R.stoi(x, x, 16000) - 1.0) < 1e-12
    assert abs(R.stoi(x, 3.0 * x, 16000) - R.stoi(x, x, 16000)) < 1e-12


def test_stoi_is_nan_below_30_frames():
    rng = np.random.default_rng(1)
    for n in (0, 100, 256, 257, 128 * 29 + 256):           # <= 29 band frames after compaction
        x = R.speech_like(rng, n, 10000, gaps=False) if n else np.zeros(0)
        assert np.isnan(R.stoi(x, x, 10000)), n
    x = R.speech_like(rng, 128 * 31 + 257, 10000, gaps=False)
    _, parts = R.stoi(x, x, 10000, return_parts=True)
    assert parts["keep"].all() and parts["env_ref"].shape[0] == 31 and parts["d"].shape[0] == 2


def test_stoi_falls_as_noise_rises():
    rng = np.random.default_rng(2)
    x = R.speech_like(rng, 16000 * 3, 16000)
    scores = [R.stoi(x, R.add_noise(rng, x, snr), 16000) for snr in (10, 5, 0, -5)]
    assert all(a > b for a, b in zip(scores, scores[1:])), scores
    assert 0.3 < scores[-1] < scores[0] < 1.0


def test_zero_estimate_follows_matlab_semantics():
    """sum Y^2 = 0 over a segment: alpha = inf, inf * 0 = NaN, min ignores it: d = corr(X, X (1 + c)) = 1."""
    rng = np.random.default_rng(4)
    x = R.speech_like(rng, 10000 * 2, 10000, gaps=False)
    _, parts = R.stoi(x, np.zeros_like(x), 10000, return_parts=True)
    assert np.allclose(parts["d"], 1.0, atol=1e-12)
    z = np.zeros(10000 * 2)
    assert np.isnan(R.stoi(z, z, 10000))                  # every frame -inf dB: nothing kept


def _declared():
    src = open(HDR).read()
    return set(re.findall(r"\b(drnmf_stoi[a-z0-9_]*)\s*\(", src))


def test_score_header_is_plain_c_and_matches_the_binding(capi, tmp_path):
    declared = _declared()
    assert declared == set(capi.SCORE_SIGNATURES), declared ^ set(capi.SCORE_SIGNATURES)
    assert not (declared & set(capi.SIGNATURES)) and not (declared & set(capi.LSTM_SIGNATURES))
    assert "drnmf_stoi" not in open(os.path.join(ROOT, "include", "drnmf.h")).read()
    L = capi.lib()
    for name in sorted(declared):
        assert hasattr(L, name), "libdrnmf.so does not export %s" % name
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "no C compiler"
    src = tmp_path / "score_header_check.c"
    src.write_text('#include "drnmf_score.h"\ntypedef void (*fn_t)(void);\nstatic const fn_t refs[] = {\n' +
                   "".join("    (fn_t)%s,\n" % n for n in sorted(declared)) +
                   "};\nint main(void) { return refs[0] != 0 ? 0 : 1; }\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_frame_counts_match_the_reference(capi):
    L = capi.lib()
    for fs in (8000, 10000, 16000, 32000, 48000):
        for n in (0, 255, 300, 4000, 16000 * 3 + 17):
            x10 = R.resample(np.ones(n), fs)
            assert L.drnmf_stoi_vad_frames(n, fs) == len(R.frame_starts(len(x10))), (fs, n)
    for fs in (0, -16000, 44100, 22050, 11025):
        assert L.drnmf_stoi_vad_frames(1000, fs) == -1
        assert L.drnmf_stoi_workspace_bytes(1, 1000, fs) == 0
    assert L.drnmf_stoi_workspace_bytes(0, 1000, 16000) == 0


def test_stoi_validates_without_a_gpu(capi):
    """On a drnmf_create_unbound handle: bad arguments -> DRNMF_ERR_INVALID_ARG, an unsupported fs ->
    DRNMF_ERR_UNSUPPORTED, a short workspace -> DRNMF_ERR_WORKSPACE, all before anything is enqueued."""
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)          # never dereferenced: validation fails first
        lens = (ctypes.c_int64 * 3)(16000, 12000, 9000)
        need = L.drnmf_stoi_workspace_bytes(3, 16000, 16000)
        assert need > 3 * 2 * 10000 * 4

        def call(n_sig=3, stride=16000, lengths=lens, fs=16000, est=fake, ref=fake, out=fake, ws=fake, nb=need,
                 handle=h):
            return L.drnmf_stoi(handle, n_sig, stride, lengths, fs, est, ref, out, None, None, None, ws, nb, None)

        assert call(handle=None) == -1
        assert call(n_sig=0) == -1
        assert call(stride=0) == -1
        assert call(lengths=None) == -1
        assert call(est=None) == -1 and call(ref=None) == -1 and call(out=None) == -1 and call(ws=None) == -1
        assert call(stride=12000) == -1                       # lengths[0] > stride
        assert b"lengths[0]" in L.drnmf_last_error(h)
        neg = (ctypes.c_int64 * 3)(16000, -1, 9000)
        assert call(lengths=neg) == -1
        for fs in (44100, 22050, 0, -8000):
            assert call(fs=fs) == -2, fs                      # DRNMF_ERR_UNSUPPORTED
        assert b"fs" in L.drnmf_last_error(h)
        assert call(nb=need - 1) == -4                        # DRNMF_ERR_WORKSPACE
        assert b"workspace" in L.drnmf_last_error(h)
        need10 = L.drnmf_stoi_workspace_bytes(3, 16000, 10000)
        assert 0 < need10 < need                              # no resampled copies at 10 kHz
        assert call(fs=10000, nb=need10 - 1) == -4
    finally:
        L.drnmf_destroy(h)
