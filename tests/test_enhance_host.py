"""CPU-side tests of the ragged enhancement path: the C ABI of include/drnmf_enhance.h and its argument
validation, the slab rule `predict` and `enhance` share, and the zero-extension identity of the reference's
framing that the GPU tests lean on (no GPU needed)."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import drnmf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_enhance.h")
NAMES = {"drnmf_stft_ragged", "drnmf_istft_ragged_workspace_bytes", "drnmf_istft_ragged",
         "drnmf_wav_int16_rows_workspace_bytes", "drnmf_wav_int16_rows"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return set(re.findall(r"\b(drnmf_[a-z0-9_]+)\s*\(", src))


def test_enhance_header_is_plain_c_and_matches_the_binding(capi, tmp_path):
    declared = _declared()
    assert declared == NAMES
    assert declared == set(capi.ENHANCE_SIGNATURES), declared ^ set(capi.ENHANCE_SIGNATURES)
    for other in (capi.SIGNATURES, capi.LSTM_SIGNATURES, capi.SCORE_SIGNATURES):
        assert not (declared & set(other))
    drnmf_h = open(os.path.join(ROOT, "include", "drnmf.h")).read()
    assert not any(n in drnmf_h for n in ("drnmf_stft_ragged", "drnmf_istft_ragged", "drnmf_wav_int16_rows"))
    L = capi.lib()
    for name in sorted(declared):
        fn = getattr(L, name)                 # exported ...
        assert fn.argtypes == capi.ENHANCE_SIGNATURES[name][1]       # ... and bound by _capi.lib()
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "no C compiler"
    src = tmp_path / "enhance_header_check.c"
    src.write_text('#include "drnmf_enhance.h"\ntypedef void (*fn_t)(void);\nstatic const fn_t refs[] = {\n' +
                   "".join("    (fn_t)%s,\n" % n for n in sorted(declared)) +
                   "};\nint main(void) { return refs[0] != 0 ? 0 : 1; }\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_workspace_queries(capi):
    L = capi.lib()
    for N, hop in ((512, 128), (1024, 256), (512, 512), (1024, 1)):
        assert L.drnmf_istft_ragged_workspace_bytes(250, 2016, N, hop) == 0          # the fused path
    assert L.drnmf_istft_ragged_workspace_bytes(3, 40, 64, 16) >= 3 * 40 * 64 * 4
    assert L.drnmf_istft_ragged_workspace_bytes(3, 40, 512, 513) >= 3 * 40 * 512 * 4   # hop > N: two stages
    assert L.drnmf_istft_ragged_workspace_bytes(0, 40, 64, 16) == 0
    assert L.drnmf_wav_int16_rows_workspace_bytes(12) >= 12 * 4
    assert L.drnmf_wav_int16_rows_workspace_bytes(0) == 0


def test_ragged_entry_points_validate_without_a_gpu(capi):
    """On a drnmf_create_unbound handle every bad argument returns DRNMF_ERR_INVALID_ARG (a short workspace
    DRNMF_ERR_WORKSPACE) with a message, before anything is enqueued."""
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)          # never dereferenced: validation fails first

        def stft(handle=h, n_sig=3, stride=1001, lengths=fake, b=2, idx=fake, T=32, N=512, hop=128, pcm=fake,
                 x=fake, re_=fake, im=fake):
            return L.drnmf_stft_ragged(handle, n_sig, stride, lengths, b, idx, T, N, hop, 1, -1.0, pcm, x, re_, im,
                                       None)

        assert stft(handle=None) == -1
        for kw in (dict(n_sig=0), dict(stride=0), dict(b=0), dict(b=65536), dict(T=0), dict(hop=0), dict(hop=-4)):
            assert stft(**kw) == -1, kw
        assert b"stft_ragged" in L.drnmf_last_error(h)
        for N in (0, 32, 48, 500, 8192, -512):
            assert stft(N=N) == -1, N
        assert b"power of two" in L.drnmf_last_error(h)
        for kw in (dict(lengths=None), dict(idx=None), dict(pcm=None), dict(x=None), dict(re_=None),
                   dict(im=None)):
            assert stft(**kw) == -1, kw
        assert b"NULL" in L.drnmf_last_error(h)

        need64 = L.drnmf_istft_ragged_workspace_bytes(2, 32, 64, 16)

        def istft(handle=h, n_sig=3, b=2, T=32, N=512, hop=128, lengths=fake, idx=fake, re_=fake, im=fake,
                  mask=fake, ld=257, y=fake, stride_y=1024, crop=0, ws=None, nb=0):
            return L.drnmf_istft_ragged(handle, n_sig, b, T, N, hop, lengths, idx, re_, im, mask, ld, y, stride_y,
                                        crop, ws, nb, None)

        assert istft(handle=None) == -1
        for kw in (dict(n_sig=0), dict(b=0), dict(b=65536), dict(T=0), dict(hop=0), dict(stride_y=0),
                   dict(crop=2), dict(crop=-1)):
            assert istft(**kw) == -1, kw
        for N in (0, 32, 48, 500, 8192):
            assert istft(N=N) == -1, N
        for kw in (dict(lengths=None), dict(idx=None), dict(re_=None), dict(im=None), dict(y=None)):
            assert istft(**kw) == -1, kw
        assert istft(ld=256) == -1                               # a mask row shorter than F
        assert b"ld_mask" in L.drnmf_last_error(h)
        assert istft(N=64, hop=16, ld=33, ws=None, nb=0) == -4   # DRNMF_ERR_WORKSPACE
        assert istft(N=64, hop=16, ld=33, ws=fake, nb=need64 - 1) == -4
        assert b"workspace" in L.drnmf_last_error(h)

        need = L.drnmf_wav_int16_rows_workspace_bytes(3)

        def rows(handle=h, n_sig=3, stride=1000, lengths=fake, y=fake, out=fake, ws=fake, nb=need):
            return L.drnmf_wav_int16_rows(handle, n_sig, stride, lengths, y, out, ws, nb, None)

        assert rows(handle=None) == -1
        for kw in (dict(n_sig=0), dict(n_sig=65536), dict(stride=0), dict(lengths=None), dict(y=None),
                   dict(out=None), dict(ws=None)):
            assert rows(**kw) == -1, kw
        assert rows(nb=need - 1) == -4
        assert b"workspace" in L.drnmf_last_error(h)
    finally:
        L.drnmf_destroy(h)


def _brute_slabs(lens, bs, step, T_cap):
    """The slab rule restated: repeatedly take the longest remaining rows (earliest index first among equals)."""
    left = list(range(len(lens)))
    slabs = []
    while left:
        left.sort(key=lambda i: (-int(lens[i]), i))
        take, left = left[:bs], left[bs:]
        T = step
        while T < max(int(lens[i]) for i in take):
            T += step
        slabs.append((take, T if T_cap is None else min(T, T_cap)))
    return slabs


def test_slab_helper_against_a_restatement(capi):
    from drnmf_amd import layers
    M = layers._SequenceModel
    step = M.PREDICT_T_STEP
    rng = np.random.default_rng(5)
    for trial in range(40):
        n = int(rng.integers(1, 70))
        bs = int(rng.integers(1, 20))
        lens = rng.integers(0, 400, size=n) if trial % 3 else rng.integers(1, 4, size=n) * 32
        cap = None if trial % 2 else int(lens.max())
        slabs = M.length_sorted_slabs(lens, bs, cap)
        seen = np.concatenate([idx for idx, _ in slabs])
        assert sorted(seen.tolist()) == list(range(n))                      # every index once
        assert np.all(np.diff(lens[seen]) <= 0)                             # non-increasing in length
        assert all(len(idx) == bs for idx, _ in slabs[:-1]) and 1 <= len(slabs[-1][0]) <= bs
        for idx, T in slabs:
            longest = int(lens[idx].max())
            if cap is None:
                assert T % step == 0 and T >= max(longest, 1) and T - step < max(longest, 1)
            else:
                assert longest <= T <= cap and (T % step == 0 or T == cap)
        want = _brute_slabs(lens, bs, step, cap)
        assert [(list(map(int, idx)), T) for idx, T in slabs] == want


def test_predict_forms_its_slabs_with_the_helper(capi):
    from drnmf_amd import layers
    src = inspect.getsource(layers._SequenceModel.predict)
    assert "length_sorted_slabs" in src and "argsort" not in src


@pytest.mark.parametrize("N,hop", [(512, 128), (1024, 256), (64, 16)])
def test_zero_extension_identity_of_the_framing(N, hop):
    """For a signal of n samples: n_frames = ceil(n/hop) + N/hop + 1, reconstruct returns ceil(n/hop) * hop
    samples, and the STFT of the zero-extended signal (a row of a ragged batch, padded to the longest) equals
    the signal's own STFT in its first n_frames frames and is exactly zero behind them."""
    rng = np.random.default_rng(N + hop)
    w = O.sqrt_hann(N)
    for n in (1, hop - 1, hop, hop + 1, 3 * hop + 7, 16001):
        x = (0.3 * rng.standard_normal(n)).astype(np.float32)
        nf = O.stft_frames(n, N, hop)
        assert nf == -(-n // hop) + N // hop + 1
        S = O.stft_mc(x, N, hop, w)
        assert S.shape == (N // 2 + 1, nf)
        y = O.reconstruct(S.real, S.imag, None, hop, w)
        assert y.shape[0] == -(-n // hop) * hop
        ext = np.concatenate([x, np.zeros(5 * hop + 3, np.float32)])
        Se = O.stft_mc(ext, N, hop, w)
        assert Se.shape[1] > nf
        assert np.max(np.abs(Se[:, :nf] - S)) == 0.0
        assert np.max(np.abs(Se[:, nf:])) == 0.0


def test_out_lengths_follow_the_oracle(capi):
    from drnmf_amd import ops
    for N, hop in ((512, 128), (1024, 256), (64, 16)):
        lens = np.array([1, hop - 1, hop, hop + 1, 3 * hop + 7, 9999, 16001])
        assert ops.ragged_out_lengths(lens, N, hop).tolist() == [-(-int(n) // hop) * hop for n in lens]
        assert ops.ragged_out_lengths(lens, N, hop, crop=True).tolist() == lens.tolist()
        L = capi.lib()
        for n in lens:
            assert L.drnmf_stft_frames(int(n), N, hop) == O.stft_frames(int(n), N, hop)


def test_enhance_checks_the_fault_word_after_its_last_copy(capi):
    """enhance cannot run without a device (pinned staging), so the order is read off the code: the stream is
    synchronised behind the device-to-host copy, then ops.check_status, then the host arrays are cut."""
    from drnmf_amd import layers
    src = inspect.getsource(layers._SequenceModel.enhance)
    i_copy = src.index("back.copy_(res")
    i_sync = src.index("synchronize()", i_copy)
    i_check = src.index("ops.check_status(dev)")
    i_cut = src.index("back.numpy()")
    assert i_copy < i_sync < i_check < i_cut


def test_enhance_rejects_before_touching_the_device(capi):
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

    w = [np.zeros(1000, np.int16)]
    with pytest.raises(ValueError, match="bins"):
        Fake(False).enhance(w, N=1024, hop=256)
    with pytest.raises(NotImplementedError):
        Fake(True).enhance(w, N=512, hop=128)
    with pytest.raises(ValueError, match="dtype"):
        Fake(False).enhance(w, dtype="float64")
    with pytest.raises(ValueError):
        Fake(False).enhance([np.zeros(1000, np.float64)])
    with pytest.raises(ValueError):
        Fake(False).enhance([np.zeros(0, np.int16)])
    with pytest.raises(ValueError):
        Fake(False).enhance(np.zeros((2, 100), np.int16))            # 2-D without lengths=
