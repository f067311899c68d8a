"""CPU-side tests of the STOI criterion: the fp64 restatement of tests/stoi_loss_ref.py against tests/stoi_ref.py
(the loss) and against central differences of it (the gradient), the C ABI of include/drnmf_stoi_loss.h and its
argument validation on a handle bound to no device, and the checks the Python layers make before they touch a device
(no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import stoi_ref as SR
import stoi_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_stoi_loss.h")
NAMES = {"drnmf_stoi_loss_workspace_bytes", "drnmf_stoi_loss"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


# ---- the restatement ------------------------------------------------------------------------------------------------
def test_loss_is_minus_the_reference_stoi_and_the_table_holds():
    for case in R.CASES:
        x, y = R.pair(*case)
        ref = SR.stoi(x, y, case[2])
        loss, counted, g = R.stoi_loss(x, y, case[2])
        assert g.shape == (case[1],)
        if (case[0], case[1]) in R.EXPECTED:
            assert counted and abs(loss - R.EXPECTED[(case[0], case[1])]) <= 5e-6, (case, loss)
        if np.isfinite(ref):
            assert counted and abs(loss + ref) <= 1e-12, (case, loss, ref)
        else:
            assert not counted and loss == 0.0 and np.all(g == 0.0), case
    # the 30-frame edge: one segment at 6554 (4097 at 10 kHz), none one sample below
    counted = {(c[1], c[2]): R.stoi_loss(*R.pair(*c), c[2])[1] for c in R.CASES if c[0] == 6}
    assert counted == {(6554, 16000): True, (6553, 16000): False, (4097, 10000): True, (4096, 10000): False}
    assert not R.stoi_loss(*R.pair(*R.CASES[4]), 16000)[1]


def _directional(x, y, fs, g, rng, zero=None):
    v = rng.standard_normal(len(y))
    if zero is not None:
        v[zero[0]:zero[1]] = 0.0
    v /= np.linalg.norm(v)
    y64 = y.astype(np.float64)
    eps = 1e-5 * np.linalg.norm(y64)
    num = -(SR.stoi(x, y64 + eps * v, fs) - SR.stoi(x, y64 - eps * v, fs)) / (2.0 * eps)
    ana = float(g @ v)
    return abs(num - ana) / abs(num), num, ana


@pytest.mark.parametrize("case", R.CASES[:4], ids=["seed%d" % c[0] for c in R.CASES[:4]])
def test_gradient_matches_central_differences(case):
    x, y = R.pair(*case)
    _, counted, g = R.stoi_loss(x, y, case[2])
    assert counted
    rng = np.random.default_rng(100 + case[0])
    for _ in range(2):
        err, num, ana = _directional(x, y, case[2], g, rng)
        print("seed %d fs %d: directional derivative %.9e (central differences %.9e), off by %.2e" %
              (case[0], case[2], ana, num, err))
        assert err <= 1e-6, (case, err)


def test_gradient_with_a_silent_stretch_of_the_estimate():
    """y[3000:9000] = 0: the segments inside the stretch have Sy == 0 (scored 1, no gradient), those at its edges
    hold zero envelopes; the gradient stays finite and matches along a direction that leaves the stretch silent."""
    x, y = R.stretch_pair()
    loss, counted, g = R.stoi_loss(x, y, 16000)
    assert counted and abs(loss + 0.74955) <= 5e-6 and np.all(np.isfinite(g))
    err, num, ana = _directional(x, y, 16000, g, np.random.default_rng(9), zero=(2600, 9400))
    print("stretch: directional derivative %.9e (central differences %.9e), off by %.2e" % (ana, num, err))
    assert err <= 1e-6


def test_all_zero_estimate_scores_one_with_no_gradient():
    x, _ = R.pair(*R.CASES[1])
    loss, counted, g = R.stoi_loss(x, np.zeros_like(x), 16000)
    assert counted and loss == -1.0 and np.all(g == 0.0)


def test_the_two_float32_roundings_of_the_device_stay_inside_the_gpu_bounds():
    """The restatement with the float32 envelopes and the float32 g of the device pipeline, against itself in
    fp64: the part of the device's error that the number formats alone explain, per sampling rate, must lie inside
    the bounds tests/test_gpu_stoi_loss.py asserts (8 x the device's measured error, rounded up to a power of ten)."""
    bounds = {10000: 1e-6, 16000: 1e-5, 8000: 1e-5}
    worst = dict.fromkeys(bounds, 0.0)
    pairs = [(R.pair(*c), c[2]) for c in R.CASES] + [(R.stretch_pair(), 16000)]
    for (x, y), fs in pairs:
        loss, counted, g = R.stoi_loss(x, y, fs)
        l32, c32, g32 = R.stoi_loss(x, y, fs, device_roundings=True)
        assert c32 == counted
        if counted:
            assert abs(l32 - loss) <= 1e-6 * abs(loss)
            worst[fs] = max(worst[fs], R.rel_err(g32, g))
    for fs, w in worst.items():
        print("fs %d: float32 envelopes and float32 g move the gradient by %.3e of max|ref|" % (fs, w))
        assert 0.0 < w <= bounds[fs], (fs, w)


def test_resample_vjp_is_the_transpose():
    rng = np.random.default_rng(5)
    for fs, n in ((16000, 700), (8000, 333), (10000, 50)):
        a, m = rng.standard_normal(n), len(SR.resample(np.zeros(n), fs))
        b = rng.standard_normal(m)
        lhs, rhs = float(SR.resample(a, fs) @ b), float(a @ R.resample_vjp(b, n, fs))
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (fs, lhs, rhs)


# ---- the C ABI ----------------------------------------------------------------------------------------------------
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return set(re.findall(r"\b(drnmf_[a-z0-9_]+)\s*\(", src))


def test_header_is_plain_c_and_matches_the_binding(capi, tmp_path):
    declared = _declared()
    assert declared == NAMES
    assert declared == set(capi.STOI_LOSS_SIGNATURES), declared ^ set(capi.STOI_LOSS_SIGNATURES)
    assert capi.STOI_LOSS_SIGNATURES in capi.SIGNATURE_TABLES
    for t in dir(capi):
        if t.endswith("SIGNATURES") and t != "STOI_LOSS_SIGNATURES":
            assert not (declared & set(getattr(capi, t))), t
    for hdr in os.listdir(os.path.join(ROOT, "include")):
        if hdr != "drnmf_stoi_loss.h":
            assert "drnmf_stoi_loss" not in open(os.path.join(ROOT, "include", hdr)).read(), hdr
    L = capi.lib()
    for name in sorted(declared):
        fn = getattr(L, name)
        assert fn.argtypes == capi.STOI_LOSS_SIGNATURES[name][1] and fn.restype == capi.STOI_LOSS_SIGNATURES[name][0]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in declared:
        assert name in doc, name
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "no C compiler"
    src = tmp_path / "stoi_loss_header_check.c"
    src.write_text('#include "drnmf_stoi_loss.h"\ntypedef void (*fn_t)(void);\nstatic const fn_t refs[] = {\n' +
                   "".join("    (fn_t)%s,\n" % n for n in sorted(declared)) +
                   "};\nint main(void) { return refs[0] != 0 && DRNMF_STOI_LOSS_STOI == %d ? 0 : 1; }\n"
                   % capi.STOI_LOSS_STOI)
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_stoi_loss_workspace_bytes(capi):
    L = capi.lib()
    for n_sig, max_len, fs in ((0, 100, 16000), (-1, 100, 16000), (3, -1, 16000), (3, 2 ** 30 + 1, 16000),
                               (3, 1000, 0), (3, 1000, 44100), (3, 1000, -8000)):
        assert L.drnmf_stoi_loss_workspace_bytes(n_sig, max_len, fs) == 0, (n_sig, max_len, fs)
    for n_sig, max_len, fs in ((1, 0, 16000), (1, 100, 10000), (1, 4097, 10000), (4, 12000, 16000), (2, 6000, 8000),
                               (64, 160000, 16000), (3, 48000, 48000)):
        b = L.drnmf_stoi_loss_workspace_bytes(n_sig, max_len, fs)
        assert b % 256 == 0 and b >= L.drnmf_stoi_workspace_bytes(n_sig, max_len, fs) > 0, (n_sig, max_len, fs, b)


def test_entry_point_validates_without_a_gpu(capi):
    """On a drnmf_create_unbound handle, with device pointers that are never dereferenced: bad arguments give
    DRNMF_ERR_INVALID_ARG (-1) with the entry's name, an unsupported fs or kind DRNMF_ERR_UNSUPPORTED (-2), a short
    or NULL workspace DRNMF_ERR_WORKSPACE (-4); of two faults the earlier check wins; a valid call stops only at
    the missing device."""
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)
        lens = (ctypes.c_int64 * 3)(5000, 12000, 0)
        need = L.drnmf_stoi_loss_workspace_bytes(3, 12000, 16000)

        def call(handle=h, n_sig=3, stride=12000, ln=lens, fs=16000, est=fake, ref=fake, kind=0, lo=fake, co=fake,
                 g=fake, sums=fake, ws=fake, ws_bytes=need):
            return L.drnmf_stoi_loss(handle, n_sig, stride, ln, fs, est, ref, kind, lo, co, g, sums, ws, ws_bytes,
                                     None)

        def err():
            return L.drnmf_last_error(h)

        assert call(handle=None) == -1
        for kw in (dict(n_sig=0), dict(n_sig=-3), dict(n_sig=65536), dict(stride=0), dict(stride=-5),
                   dict(stride=2 ** 38 + 1)):
            assert call(**kw) == -1 and b"stoi_loss: bad argument" in err(), kw
        for name in ("ln", "est", "ref", "lo", "co", "g", "sums"):
            assert call(**{name: None}) == -1 and b"stoi_loss: bad argument" in err(), name
        assert call(stride=11999) == -1 and b"stoi_loss: lengths[1] = 12000" in err()
        assert call(ln=(ctypes.c_int64 * 3)(5, -1, 7)) == -1 and b"stoi_loss: lengths[1] = -1" in err()
        for fs in (0, -16000, 44100, 11025):
            assert call(fs=fs) == -2 and b"stoi_loss: fs = " in err(), fs
        for kind in (1, -1, 7):
            assert call(kind=kind) == -2 and b"stoi_loss: kind = " in err(), kind
        for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
            assert call(**kw) == -4 and b"stoi_loss: workspace too small" in err(), kw
        assert call(ws=ctypes.c_void_p(0x100008)) == -4 and b"256-byte aligned" in err()
        assert call(est=None, fs=0) == -1                                   # arguments before fs
        assert call(fs=0, kind=3) == -2 and b"fs = " in err()               # fs before kind
        assert call(kind=3, ws=None) == -2 and b"kind = " in err()          # kind before workspace
        for fs, ln in ((16000, lens), (10000, lens), (8000, lens), (48000, lens)):
            nb = L.drnmf_stoi_loss_workspace_bytes(3, 12000, fs)
            assert call(fs=fs, ws_bytes=nb) not in (0, -1, -2, -4) and b"no device" in err(), fs
    finally:
        L.drnmf_destroy(h)


# ---- the Python layers ---------------------------------------------------------------------------------------------
def test_ops_refuse_before_the_device_is_touched(capi):
    from drnmf_amd import ops
    z = torch.zeros((2, 5000))
    with pytest.raises(ValueError, match="no CPU"):
        ops.stoi_loss(z, z, [5000, 4000])
    with pytest.raises(ValueError, match="est, ref"):
        ops.stoi_loss(z, torch.zeros((2, 5001)), [5000, 4000])
    with pytest.raises(ValueError, match="est, ref"):
        ops.stoi_loss(z.double(), z.double(), [5000, 4000])
    with pytest.raises(ValueError, match="loss must be one of"):
        ops.wave_loss(z, z, [10, 10], loss="stoi")                  # (the C constants of drnmf_wave_loss are two)
    assert ops.WAVE_LOSSES == {"wave_mse": 0, "si_sdr": 1} and ops.WAVE_CRITERIA == ("si_sdr", "wave_mse", "stoi")


def test_models_refuse_before_the_device_is_touched(capi):
    from drnmf_amd import layers
    a, b = np.zeros(1000, np.float32), np.zeros(700, np.float32)

    class Fake(layers._SequenceModel):
        mask_value = -1.0

        def __init__(self, stateful=False, compiled=True):
            self._st = stateful
            if compiled:
                self._flat = None

        def _device(self):
            return "cuda:0"

        def _input_width(self):
            return 33

        def _stateful(self):
            return self._st

    for call in ("train_on_wavs", "test_on_wavs", "fit_waveform"):
        with pytest.raises(ValueError, match=r"loss must be one of \['si_sdr', 'wave_mse', 'stoi'\]"):
            getattr(Fake(), call)([a], [b], loss="sdr", N=64, hop=16)
        with pytest.raises(NotImplementedError, match="stateful"):
            getattr(Fake(stateful=True), call)([a], [b], loss="stoi", N=64, hop=16)
        with pytest.raises(ValueError, match="bins"):
            getattr(Fake(), call)([a], [b], loss="stoi", N=128, hop=16)
        with pytest.raises(ValueError, match="fs = 44100"):
            getattr(Fake(), call)([a], [b], loss="stoi", N=64, hop=16, fs=44100)
        with pytest.raises(ValueError, match=call):                 # fs is ignored by the other criteria
            getattr(Fake(), call)([], [b], loss="si_sdr", N=64, hop=16, fs=44100)
    for call in ("train_on_wavs", "fit_waveform"):
        with pytest.raises(ValueError, match="compile"):
            getattr(Fake(compiled=False), call)([a], [b], loss="stoi", N=64, hop=16)
    model = layers.build_snmf(dict(r=4, sparsity=0.1, cf='ed', max_iter=2, conv_eps=0., random_seed=1),
                              np.ones((33, 8), np.float32), device="cpu")
    for call in ("train_on_wavs", "test_on_wavs", "fit_waveform"):
        with pytest.raises(NotImplementedError, match="SparseNMFModel"):
            getattr(model, call)([a], [b], loss="stoi", N=64, hop=16)
