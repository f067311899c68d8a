"""CPU-side tests of the training-data front end: the C ABI of include/drnmf_dataset.h and its argument
validation, the sequence table the device takes against reshape_and_pad_stacks, and the checks
ops.wavs_to_tensors / wavs_to_frames / fit_wavs make before they touch a device (no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_dataset.h")
NAMES = {"drnmf_stft_pair_chunks", "drnmf_stft_pair_frames"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return set(re.findall(r"\b(drnmf_[a-z0-9_]+)\s*\(", src))


def test_dataset_header_is_plain_c_and_matches_the_binding(capi, tmp_path):
    declared = _declared()
    assert declared == NAMES
    assert declared == set(capi.DATASET_SIGNATURES), declared ^ set(capi.DATASET_SIGNATURES)
    for other in (capi.SIGNATURES, capi.LSTM_SIGNATURES, capi.SCORE_SIGNATURES, capi.ENHANCE_SIGNATURES,
                  capi.SDR_SIGNATURES):
        assert not (declared & set(other))
    for hdr in ("drnmf.h", "drnmf_enhance.h", "drnmf_score.h", "drnmf_sdr.h", "drnmf_lstm.h"):
        assert "drnmf_stft_pair" not in open(os.path.join(ROOT, "include", hdr)).read(), hdr
    L = capi.lib()
    for name in sorted(declared):
        fn = getattr(L, name)                 # exported ...
        assert fn.argtypes == capi.DATASET_SIGNATURES[name][1]       # ... and bound by _capi.lib()
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "no C compiler"
    src = tmp_path / "dataset_header_check.c"
    src.write_text('#include "drnmf_dataset.h"\ntypedef void (*fn_t)(void);\nstatic const fn_t refs[] = {\n' +
                   "".join("    (fn_t)%s,\n" % n for n in sorted(declared)) +
                   "};\nint main(void) { return refs[0] != 0 && DRNMF_TRANSFORM_LOGMAG == 1 ? 0 : 1; }\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_pair_entry_points_validate_without_a_gpu(capi):
    """On a drnmf_create_unbound handle every bad argument returns DRNMF_ERR_INVALID_ARG with a message, before
    anything is enqueued."""
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)          # never dereferenced: validation fails first

        def chunks(handle=h, n_sig=3, sx=1001, sy=999, lx=fake, ly=fake, n_seq=5, table=fake, T=7, N=512, hop=128,
                   i16=1, tr=0, px=fake, py=fake, x=fake, y=fake, w=fake):
            return L.drnmf_stft_pair_chunks(handle, n_sig, sx, sy, lx, ly, n_seq, table, T, N, hop, i16, tr, -1.0,
                                            px, py, x, y, w, None)

        def frames(handle=h, n_sig=3, sx=1001, sy=999, lx=fake, ly=fake, row0=fake, total=40, N=512, hop=128,
                   i16=1, tr=0, px=fake, py=fake, x=fake, y=fake):
            return L.drnmf_stft_pair_frames(handle, n_sig, sx, sy, lx, ly, row0, total, N, hop, i16, tr, px, py, x,
                                            y, None)

        for call, who, shapes, pointers in (
                (chunks, b"stft_pair_chunks",
                 (dict(n_sig=0), dict(sx=0), dict(sy=0), dict(sx=-3), dict(n_seq=0), dict(n_seq=-1), dict(T=0),
                  dict(T=-7), dict(hop=0), dict(hop=-4), dict(i16=2)),
                 ("lx", "ly", "table", "px", "py", "x", "y", "w")),
                (frames, b"stft_pair_frames",
                 (dict(n_sig=0), dict(sx=0), dict(sy=0), dict(total=0), dict(total=-1), dict(hop=0), dict(hop=-4),
                  dict(i16=-1)),
                 ("lx", "ly", "row0", "px", "py", "x", "y"))):
            assert call(handle=None) == -1
            for kw in shapes:
                assert call(**kw) == -1, kw
                msg = L.drnmf_last_error(h)
                assert who in msg and b"bad shape" in msg, (kw, msg)
            for N in (0, 32, 48, 500, 8192, -512):
                assert call(N=N) == -1, N
                assert who in L.drnmf_last_error(h) and b"power of two" in L.drnmf_last_error(h)
            for tr in (-1, 2, 7):
                assert call(tr=tr) == -1, tr
                assert who in L.drnmf_last_error(h) and b"transform" in L.drnmf_last_error(h)
            for name in pointers:
                assert call(**{name: None}) == -1, name
                assert who in L.drnmf_last_error(h) and b"NULL" in L.drnmf_last_error(h)
            assert call(sy=2 ** 40, hop=1) == -1                     # more frames than an int32 counts
            assert b"frames" in L.drnmf_last_error(h)
    finally:
        L.drnmf_destroy(h)


def _check_table(n_frames, maxlen):
    from drnmf_amd import data
    n_frames = np.asarray(n_frames, dtype=np.int64)
    table, T = data.sequence_table_from_lengths(n_frames, maxlen)
    assert table.dtype == np.int32 and table.ndim == 2 and table.shape[1] == 2
    ends = np.cumsum(n_frames)
    fidx = np.stack([ends - n_frames, ends], axis=1)
    # a stack whose columns are numbered: reshape_and_pad_stacks then shows which frame went where
    stack = np.arange(int(ends[-1]), dtype=np.float64)[None, :]
    x, _, mask = data.reshape_and_pad_stacks(stack, stack, fidx, pad_value=-1.0, maxlen=maxlen)
    assert x.shape[0] == table.shape[0] and x.shape[1] == T
    valid = np.arange(T)[None, :] + table[:, 1:2] < n_frames[table[:, 0]][:, None]
    assert np.array_equal(mask[:, :, 0], valid.astype(np.float64))
    want = np.where(valid, fidx[table[:, 0], 0][:, None] + table[:, 1:2] + np.arange(T)[None, :], -1)
    assert np.array_equal(x[:, :, 0], want.astype(np.float64))
    assert valid[:, 0].all()                                        # no empty piece
    return table, T


def test_sequence_table_follows_reshape_and_pad_stacks(capi):
    rng = np.random.default_rng(11)
    for trial in range(30):
        n = int(rng.integers(1, 12))
        nf = rng.integers(1, 60, size=n)
        maxlen = [None, int(rng.integers(1, 70)), int(nf.max()), int(nf.max()) + 1][trial % 4]
        _check_table(nf, maxlen)


def test_sequence_table_edges(capi):
    table, T = _check_table([23], 7)                                # one utterance: 7 + 7 + 7 + 2
    assert T == 7 and table.tolist() == [[0, 0], [0, 7], [0, 14], [0, 21]]
    table, T = _check_table([3, 5, 4], 7)                           # all shorter than maxlen: T = the longest
    assert T == 5 and table.tolist() == [[0, 0], [1, 0], [2, 0]]
    table, T = _check_table([14, 7, 21], 7)                         # exact multiples: no empty trailing piece
    assert T == 7 and table.shape[0] == 2 + 1 + 3
    table, T = _check_table([3, 1, 2], 1)                           # maxlen = 1: one frame per sequence
    assert T == 1 and table.tolist() == [[0, 0], [0, 1], [0, 2], [1, 0], [2, 0], [2, 1]]
    for maxlen in (None, 10, 1000):                                 # maxlen above the longest
        table, T = _check_table([9, 4], maxlen)
        assert T == 9 and table.tolist() == [[0, 0], [1, 0]]
    from drnmf_amd import data
    for bad in (([], None), ([4, 0], None), ([4], 0)):
        with pytest.raises(ValueError):
            data.sequence_table_from_lengths(*bad)


def test_wav_pairs_are_refused_before_the_device_is_touched(capi):
    """These run on a machine without a GPU: the checks come before the first allocation."""
    from drnmf_amd import layers, ops
    a, b = np.zeros(1000, np.int16), np.zeros(700, np.int16)
    for fn in (lambda *p, **k: ops.wavs_to_tensors(*p, **k), lambda *p, **k: ops.wavs_to_frames(*p, N=512, hop=128,
                                                                                                 **k)):
        with pytest.raises(ValueError, match="noisy waveforms for"):
            fn([a, a], [a])
        with pytest.raises(ValueError, match="no waveforms"):
            fn([], [])
        with pytest.raises(ValueError, match="fewer than its clean"):
            fn([a, b], [a, a])                                      # 700 samples: 3 frames fewer than 1000
        with pytest.raises(ValueError, match="transform"):
            fn([a], [a], transform="power")
        with pytest.raises(ValueError):
            fn([a], [a.astype(np.float32)])                         # both sides of one type
        with pytest.raises(ValueError):
            fn([np.zeros((2, 10), np.int16)], [a])
    with pytest.raises(ValueError, match="power of two"):
        ops.wavs_to_tensors([a], [a], N=320, hop=160)

    class Fake(layers._SequenceModel):
        def __init__(self, mask_value):
            self.mask_value = mask_value

        def _device(self):
            return "cuda:0"

        def _input_width(self):
            return 257

    with pytest.raises(ValueError, match="masks"):
        Fake(0.0).fit_wavs([a], [a])                                # 'mag' pads with -1
    with pytest.raises(ValueError, match="bins"):
        Fake(-1.0).fit_wavs([a], [a], N=1024, hop=256)
    with pytest.raises(ValueError, match="validation_wavs"):
        Fake(-1.0).fit_wavs([a], [a], validation_data=(1, 2))
    with pytest.raises(ValueError, match="fewer than its clean"):
        Fake(-1.0).fit_wavs([b], [a])
