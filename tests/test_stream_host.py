"""CPU-side tests of the streaming path: the C ABI of include/drnmf_stream.h, the counting rule against the
offline framing (drnmf_stft_frames, ops.ragged_out_lengths) over random cut schedules, argument validation on an
unbound handle, and the checks model.stream makes before it touches a device (no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_stream.h")
NAMES = {"drnmf_stream_counts", "drnmf_stream_state_bytes", "drnmf_stream_reset", "drnmf_stream_forward",
         "drnmf_stream_inverse"}
SIZES = [(512, 128), (1024, 256), (64, 16), (512, 512)]


def lengths(hop):
    return [1, hop - 1, hop, hop + 1, 3 * hop + 7, 9999, 16001]


def pieces(N, hop):
    return [0, 1, hop - 1, hop, hop + 1, N - 1, N, N + hop + 3, 2999]


def cut_schedule(L, N, hop, rng):
    """Chunk lengths that sum to L, drawn from the piece set (the last one cut to fit)."""
    cuts, left = [], int(L)
    while left > 0:
        c = min(int(rng.choice(pieces(N, hop))), left)
        cuts.append(c)
        left -= c
    return cuts


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return set(re.findall(r"\b(drnmf_[a-z0-9_]+)\s*\(", src))


def test_stream_header_is_plain_c_and_matches_the_binding(capi, tmp_path):
    declared = _declared()
    assert declared == NAMES
    assert declared == set(capi.STREAM_SIGNATURES), declared ^ set(capi.STREAM_SIGNATURES)
    for other in (capi.SIGNATURES, capi.LSTM_SIGNATURES, capi.SCORE_SIGNATURES, capi.ENHANCE_SIGNATURES,
                  capi.SDR_SIGNATURES, capi.DATASET_SIGNATURES):
        assert not (declared & set(other))
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(HDR).read())
    assert includes == ["drnmf.h"]
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "drnmf_stream.h":
            assert "drnmf_stream" not in open(os.path.join(ROOT, "include", name)).read(), name
    L = capi.lib()
    for name in sorted(declared):
        fn = getattr(L, name)                 # exported ...
        assert fn.argtypes == capi.STREAM_SIGNATURES[name][1]        # ... and bound by _capi.lib()
        assert fn.restype == capi.STREAM_SIGNATURES[name][0]
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "no C compiler"
    src = tmp_path / "stream_header_check.c"
    src.write_text('#include "drnmf_stream.h"\ntypedef void (*fn_t)(void);\nstatic const fn_t refs[] = {\n' +
                   "".join("    (fn_t)%s,\n" % n for n in sorted(declared)) +
                   "};\nint main(void) { return refs[0] != 0 ? 0 : 1; }\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


@pytest.mark.parametrize("N,hop", SIZES)
def test_counting_rule_against_the_offline_framing(capi, N, hop):
    from drnmf_amd import ops
    L = capi.lib()
    rng = np.random.default_rng(1000 * N + hop)
    for length in lengths(hop):
        nf = L.drnmf_stft_frames(length, N, hop)
        for crop in (False, True):
            want_out = int(ops.ragged_out_lengths([length], N, hop, crop)[0])
            for trial in range(4):
                cuts = cut_schedule(length, N, hop, rng)
                if trial == 3:
                    cuts = [0] + cuts + [0]              # empty pushes in front and before the close
                n = frames = samples = 0                # a stream that has never been pushed
                for i, c in enumerate(cuts):
                    last = trial % 2 == 0 and i == len(cuts) - 1     # close with the last chunk, or separately
                    n += c
                    f, s = ops.stream_counts(n, last, N, hop, crop)
                    if not last:
                        assert f == n // hop + 1 and s == max(0, f * hop - N)
                        assert N - hop <= n - (f * hop - N) <= N - 1      # the delay of an open stream
                    assert f >= frames and s >= samples
                    frames, samples = f, s
                f, s = ops.stream_counts(n, True, N, hop, crop)          # (the separate close; else no change)
                assert f >= frames and s >= samples
                assert n == length and f == nf and s == want_out
                assert f == -(-length // hop) + N // hop + 1
                assert s == (min(length, hop * (nf - 1) - N) if crop else hop * (nf - 1) - N)


def test_counting_function_rejects_bad_arguments(capi):
    L = capi.lib()
    f, s = ctypes.c_int64(), ctypes.c_int64()
    ok = lambda *a: L.drnmf_stream_counts(*a, ctypes.byref(f), ctypes.byref(s))
    assert ok(100, 0, 512, 128, 0) == 0 and (f.value, s.value) == (1, 0)
    assert ok(0, 0, 512, 128, 0) == 0 and (f.value, s.value) == (1, 0)
    for bad in ((-1, 0, 512, 128, 0), (10, 0, 0, 128, 0), (10, 0, 512, 0, 0), (10, 0, 512, 1024, 0),
                (10, 0, 512, 96, 0), (10, 2, 512, 128, 0), (10, 0, 512, 128, 2)):
        assert ok(*bad) == -1, bad
    assert L.drnmf_stream_counts(10, 0, 512, 128, 0, None, ctypes.byref(s)) == -1
    assert L.drnmf_stream_counts(10, 0, 512, 128, 0, ctypes.byref(f), None) == -1


def test_state_size_query(capi):
    L = capi.lib()
    for N, hop in SIZES + [(4096, 1)]:
        one = L.drnmf_stream_state_bytes(1, N, hop)
        # header, fewer than N carried input samples, N - hop partial sums
        assert one >= 64 + 4 * (N - 1) + 4 * (N - hop) and one % 64 == 0
        assert L.drnmf_stream_state_bytes(7, N, hop) == 7 * one
    for bad in ((0, 512, 128), (65536, 512, 128), (1, 500, 125), (1, 32, 8), (1, 8192, 128), (1, 512, 0),
                (1, 512, 1024), (1, 512, 96)):
        assert L.drnmf_stream_state_bytes(*bad) == 0, bad


def test_stream_entry_points_validate_without_a_gpu(capi):
    """On a drnmf_create_unbound handle every bad argument returns DRNMF_ERR_INVALID_ARG with a message naming
    the entry point, before anything is enqueued."""
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)          # never dereferenced: validation fails first
        big = 1 << 30

        def reset(handle=h, B=3, N=512, hop=128, state=fake, nb=big):
            return L.drnmf_stream_reset(handle, B, N, hop, state, nb, None)

        def fwd(handle=h, B=3, stride=1000, T=8, N=512, hop=128, chunk=fake, clen=fake, fin=fake, x=fake,
                re_=fake, im=fake, state=fake, nb=big):
            return L.drnmf_stream_forward(handle, B, stride, T, N, hop, 1, -1.0, chunk, clen, fin, x, re_, im,
                                          state, nb, None)

        def inv(handle=h, B=3, T=8, N=512, hop=128, re_=fake, im=fake, mask=fake, ld=257, crop=1, i16=0, y=fake,
                stride_y=1024, state=fake, nb=big):
            return L.drnmf_stream_inverse(handle, B, T, N, hop, re_, im, mask, ld, crop, i16, y, stride_y, state,
                                          nb, None)

        def message(fn, who, **kw):
            assert (inv if fn is not inv else fwd)(B=0) == -1            # leaves another entry point's message
            assert who not in L.drnmf_last_error(h)
            assert fn(**kw) == -1, (who, kw)
            msg = L.drnmf_last_error(h)
            assert who in msg, (who, kw, msg)
            return msg

        for fn, who in ((reset, b"stream_reset"), (fwd, b"stream_forward"), (inv, b"stream_inverse")):
            assert fn(handle=None) == -1
            for B in (0, 65536):
                message(fn, who, B=B)
            for N in (0, 32, 48, 500, 8192):
                assert b"power of two" in message(fn, who, N=N, hop=1 if N < 128 else 128) or N == 0
            for hop in (0, 1024, 96, 384, -128):
                assert b"hop" in message(fn, who, hop=hop)
            assert b"NULL" in message(fn, who, state=None)
            need = L.drnmf_stream_state_bytes(3, 512, 128)
            assert b"state" in message(fn, who, nb=need - 1)
            assert b"state" in message(fn, who, nb=0)
        for fn, who in ((fwd, b"stream_forward"), (inv, b"stream_inverse")):
            message(fn, who, T=0)
            message(fn, who, T=-3)
        for kw in (dict(chunk=None), dict(clen=None), dict(fin=None), dict(x=None), dict(re_=None), dict(im=None)):
            assert b"NULL" in message(fwd, b"stream_forward", **kw)
        message(fwd, b"stream_forward", stride=0)
        for kw in (dict(re_=None), dict(im=None), dict(y=None)):
            assert b"NULL" in message(inv, b"stream_inverse", **kw)
        assert b"ld_mask" in message(inv, b"stream_inverse", ld=256)       # a mask row shorter than F
        for kw in (dict(stride_y=0), dict(crop=2), dict(i16=2)):
            message(inv, b"stream_inverse", **kw)
    finally:
        L.drnmf_destroy(h)


def test_model_stream_rejects_before_touching_the_device(capi):
    from drnmf_amd import layers

    class Fake(layers._SequenceModel):
        mask_value = -1.0

        def __init__(self, stateful):
            self.st = stateful

        def _device(self):
            return "cuda:0"

        def _input_width(self):
            return 257

        def _stateful(self):
            return self.st

    with pytest.raises(ValueError, match="stateful=True"):
        Fake(False).stream(4)
    with pytest.raises(ValueError, match="bins"):
        Fake(True).stream(4, N=1024, hop=256)
    with pytest.raises(ValueError, match="dtype"):
        Fake(True).stream(4, dtype="float64")
    assert hasattr(layers.UnfoldedSNMFModel, "stream") and hasattr(layers.LSTMModel, "stream")
    with pytest.raises(NotImplementedError):                             # enhance keeps refusing them
        Fake(True).enhance([np.zeros(1000, np.int16)], N=512, hop=128)
