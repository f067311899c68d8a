"""CPU-side tests of the device-side mixer: the C ABI of include/drnmf_mix.h and its argument validation on a
handle bound to no device, the workspace size, the host-side draw, the checks ops.MixBank / fit_mixtures /
from_mixtures make before they touch a device, and the fp64 reference against itself (no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mix_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_mix.h")
NAMES = {"drnmf_mix_workspace_bytes", "drnmf_mix_energy", "drnmf_mix_forward"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return set(re.findall(r"\b(drnmf_[a-z0-9_]+)\s*\(", src))


def test_mix_header_is_plain_c_and_matches_the_binding(capi, tmp_path):
    declared = _declared()
    assert declared == NAMES
    assert declared == set(capi.MIX_SIGNATURES), declared ^ set(capi.MIX_SIGNATURES)
    others = [getattr(capi, t) for t in dir(capi) if t.endswith("SIGNATURES") and t != "MIX_SIGNATURES"]
    assert len(others) >= 14
    for other in others:
        assert not (declared & set(other))
    for hdr in os.listdir(os.path.join(ROOT, "include")):
        if hdr != "drnmf_mix.h":
            assert "drnmf_mix_" not in open(os.path.join(ROOT, "include", hdr)).read(), hdr
    L = capi.lib()
    for name in sorted(declared):
        fn = getattr(L, name)                 # exported ...
        assert fn.argtypes == capi.MIX_SIGNATURES[name][1]       # ... and bound by _capi.lib()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in declared:
        assert name in doc, name
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "no C compiler"
    src = tmp_path / "mix_header_check.c"
    src.write_text('#include "drnmf_mix.h"\ntypedef void (*fn_t)(void);\nstatic const fn_t refs[] = {\n' +
                   "".join("    (fn_t)%s,\n" % n for n in sorted(declared)) +
                   "};\nint main(void) { return refs[0] != 0 && DRNMF_MIX_BLOCK == %d ? 0 : 1; }\n" % capi.MIX_BLOCK)
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_mix_workspace_bytes(capi):
    L = capi.lib()
    for n_sig, stride in ((0, 100), (-1, 100), (3, 0), (3, -5)):
        assert L.drnmf_mix_workspace_bytes(n_sig, stride) == 0, (n_sig, stride)
    for n_sig, stride in ((1, 1), (1, 4096), (1, 4097), (5, 10000), (70, 4095), (512, 96000), (70000, 3)):
        b = L.drnmf_mix_workspace_bytes(n_sig, stride)
        assert b > 0 and b % 256 == 0, (n_sig, stride, b)
        assert b >= 8 * (n_sig * -(-stride // 4096) + n_sig), (n_sig, stride, b)


def test_mix_entry_points_validate_without_a_gpu(capi):
    """On a drnmf_create_unbound handle: every bad shape and every required NULL pointer returns
    DRNMF_ERR_INVALID_ARG with a message, a short or NULL workspace DRNMF_ERR_WORKSPACE, and a fully valid call
    stops only at the missing device."""
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)          # never dereferenced: the call stops before any launch
        need = L.drnmf_mix_workspace_bytes(3, 1001)

        def energy(handle=h, n_sig=3, stride=1001, ln=fake, i16=1, pcm=fake, out=fake, ws=fake, ws_bytes=need):
            return L.drnmf_mix_energy(handle, n_sig, stride, ln, i16, pcm, out, ws, ws_bytes, None)

        def forward(handle=h, n_sig=3, ss=1001, ls=fake, si16=0, sp=fake, n_noise=2, sn=777, ln=fake, ni16=1, nz=fake,
                    idx=fake, off=fake, snr=fake, es=fake, noisy=fake, gain=fake, ws=fake, ws_bytes=need):
            return L.drnmf_mix_forward(handle, n_sig, ss, ls, si16, sp, n_noise, sn, ln, ni16, nz, idx, off, snr, es,
                                       noisy, gain, ws, ws_bytes, None)

        for call, who, shapes, pointers, optional in (
                (energy, b"mix_energy",
                 (dict(n_sig=0), dict(n_sig=-2), dict(stride=0), dict(stride=-7), dict(i16=2), dict(i16=-1)),
                 ("ln", "pcm", "out"), ()),
                (forward, b"mix_forward",
                 (dict(n_sig=0), dict(n_sig=-2), dict(ss=0), dict(ss=-7), dict(n_noise=0), dict(n_noise=-1),
                  dict(sn=0), dict(sn=-3), dict(si16=2), dict(si16=-1), dict(ni16=2), dict(ni16=-1)),
                 ("ls", "sp", "ln", "nz", "idx", "off", "snr", "noisy"), ("es", "gain"))):
            assert call(handle=None) == -1
            for kw in shapes:
                assert call(**kw) == -1, kw
                msg = L.drnmf_last_error(h)
                assert who in msg and b"bad shape" in msg, (kw, msg)
            for name in pointers:
                assert call(**{name: None}) == -1, name
                assert who in L.drnmf_last_error(h) and b"NULL" in L.drnmf_last_error(h)
            for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
                assert call(**kw) == -4, kw
                assert who in L.drnmf_last_error(h) and b"workspace" in L.drnmf_last_error(h)
            # everything in order: what stops the call is that the handle is bound to no device
            for kw in [dict()] + [{name: None} for name in optional]:
                rc = call(**kw)
                assert rc not in (0, -1, -2, -4) and who in L.drnmf_last_error(h) and \
                    b"no device" in L.drnmf_last_error(h), (kw, rc)
    finally:
        L.drnmf_destroy(h)


def test_draw_is_a_pure_function_of_its_arguments(capi):
    from drnmf_amd import ops
    len_noise = np.array([1, 3, 7, 4096, 5000, 50000], dtype=np.int64)
    n = 500
    a = ops.mix_draw(n, len_noise, snr_db=(-10.0, 20.0), seed=3, epoch=2)
    b = ops.mix_draw(n, len_noise, snr_db=(-10.0, 20.0), seed=3, epoch=2)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    idx, off, snr = a
    assert idx.dtype == np.int32 and off.dtype == np.int64 and snr.dtype == np.float32
    assert idx.shape == off.shape == snr.shape == (n,)
    assert idx.min() >= 0 and idx.max() < len(len_noise) and len(set(idx.tolist())) == len(len_noise)
    assert (off >= 0).all() and (off < len_noise[idx]).all()
    assert (snr >= -10.0).all() and (snr <= 20.0).all() and snr.std() > 1.0
    for other in (dict(seed=3, epoch=3), dict(seed=4, epoch=2)):
        c = ops.mix_draw(n, len_noise, snr_db=(-10.0, 20.0), **other)
        assert all(not np.array_equal(u, v) for u, v in zip(a, c)), other
    # the recipe, written out
    rs = np.random.RandomState((3 * 1000003 + 2) % 2 ** 32)
    want_idx = rs.randint(0, len(len_noise), n)
    want_off = np.minimum(np.floor(rs.random_sample(n) * len_noise[want_idx]), len_noise[want_idx] - 1)
    want_snr = -10.0 + 30.0 * rs.random_sample(n)
    assert np.array_equal(idx, want_idx) and np.array_equal(off, want_off.astype(np.int64))
    assert np.array_equal(snr, want_snr.astype(np.float32))
    # a list of SNRs
    choices = [-6.0, -3.0, 0.0, 3.0, 6.0, 9.0]
    idx2, off2, snr2 = ops.mix_draw(n, len_noise, snr_choices=choices, seed=3, epoch=2)
    assert snr2.dtype == np.float32 and set(snr2.tolist()) == set(choices)
    assert np.array_equal(idx2, idx) and np.array_equal(off2, off)
    # neither: the default range
    lo, hi = ops.MIX_SNR_DB
    snr3 = ops.mix_draw(n, len_noise)[2]
    assert (snr3 >= lo).all() and (snr3 <= hi).all()
    with pytest.raises(ValueError, match="not both"):
        ops.mix_draw(n, len_noise, snr_db=(0.0, 5.0), snr_choices=choices)
    for bad in (dict(snr_db=(5.0, 0.0)), dict(snr_db=(0.0, float("inf"))), dict(snr_choices=[]),
                dict(snr_choices=[float("nan")])):
        with pytest.raises(ValueError):
            ops.mix_draw(n, len_noise, **bad)
    with pytest.raises(ValueError):
        ops.mix_draw(n, [5, 0])
    with pytest.raises(ValueError):
        ops.mix_draw(0, len_noise)


def test_banks_are_refused_before_the_device_is_touched(capi):
    """These run on a machine without a GPU: the checks come before the first allocation."""
    from drnmf_amd import layers, ops
    a, b = np.zeros(1000, np.int16), np.zeros(700, np.float32)
    bad_sides = ([], [a, b], [a.astype(np.float64)], [np.zeros((2, 10), np.int16)], [a, np.zeros(0, np.int16)])
    params = dict(r=4, sparsity=0.1, cf='ed', max_iter=2, conv_eps=0., random_seed=1)
    for bad in bad_sides:
        for clean, noise in ((bad, [a]), ([a], bad)):
            with pytest.raises(ValueError, match="MixBank"):
                ops.MixBank(clean, noise)
            with pytest.raises(ValueError, match="from_mixtures"):
                layers.SparseNMFModel.from_mixtures(clean, noise, params, N=64, hop=16)
    with pytest.raises(ValueError, match="not both"):
        layers.SparseNMFModel.from_mixtures([a], [a], params, snr_db=(0., 3.), snr_choices=[1.0])

    class Fake(layers._SequenceModel):
        def __init__(self, mask_value):
            self.mask_value = mask_value

        def _device(self):
            return "cuda:0"

        def _input_width(self):
            return 257

    with pytest.raises(ValueError, match="masks"):
        Fake(0.0).fit_mixtures([a], [a])                            # 'mag' pads with -1
    with pytest.raises(ValueError, match="bins"):
        Fake(-1.0).fit_mixtures([a], [a], N=1024, hop=256)
    with pytest.raises(ValueError, match="validation_wavs"):
        Fake(-1.0).fit_mixtures([a], [a], validation_data=(1, 2))
    with pytest.raises(ValueError, match="validation_wavs"):
        Fake(-1.0).fit_mixtures([a], [a], sample_weight=1)
    with pytest.raises(ValueError, match="target"):
        Fake(-1.0).fit_mixtures([a], [a], target='irm')
    with pytest.raises(ValueError, match="not both"):
        Fake(-1.0).fit_mixtures([a], [a], snr_db=(0., 3.), snr_choices=[1.0])
    for bad in bad_sides:
        with pytest.raises(ValueError, match="fit_mixtures"):
            Fake(-1.0).fit_mixtures(bad, [a])
        with pytest.raises(ValueError, match="fit_mixtures"):
            Fake(-1.0).fit_mixtures([a], bad)
    model = layers.build_snmf(params, np.ones((33, 8), np.float32), device="cpu")
    with pytest.raises(NotImplementedError, match="from_mixtures"):
        model.fit_mixtures([a], [a])


def test_the_reference_realises_its_own_snr():
    rng = np.random.default_rng(5)
    worst = 0.0
    for trial in range(60):
        n = int(rng.choice([1, 2, 7, 4095, 4096, 4097, 10000]))
        L = int(rng.choice([1, 3, 7, 4096, 5000, 50000]))
        sc = float(rng.choice([1e-3, 0.1, 0.5]))
        if trial % 2:
            s = (sc * rng.standard_normal(n)).astype(np.float32)
            z = (float(rng.choice([1e-3, 0.1, 0.5])) * rng.standard_normal(L)).astype(np.float32)
        else:
            s = np.clip(np.round(sc * 32768 * rng.standard_normal(n)), -32768, 32767).astype(np.int16)
            z = np.clip(np.round(0.1 * 32768 * rng.standard_normal(L)), -32768, 32767).astype(np.int16)
            s[0], z[0] = 11, 7                  # never all-zero
        snr = float(rng.uniform(-10, 20))
        off = int(rng.choice([0, L - 1, L // 2, -3, L + 5]))
        g, noisy, seg = R.mix_one(s, z, off, snr)
        assert g > 0 and noisy.shape == (n,)
        assert np.array_equal(seg, R.as_float(z)[(off % L + np.arange(n)) % L])
        worst = max(worst, abs(R.realised_snr_db(R.as_float(s), noisy) - snr))
    assert worst <= 1e-9, worst
    # the degenerate rows
    s = (0.1 * rng.standard_normal(50)).astype(np.float32)
    z = (0.1 * rng.standard_normal(20)).astype(np.float32)
    for args in ((np.zeros(50, np.float32), z, 0, 3.0), (s, np.zeros(20, np.float32), 0, 3.0), (s, None, 0, 3.0),
                 (s, z, 0, float("nan")), (s, z, 0, float("inf")), (s, z, 0, float("-inf"))):
        g, noisy, _ = R.mix_one(*args)
        assert g == 0.0 and np.array_equal(noisy, R.as_float(args[0]))
