"""CPU-side tests of the device-side reverberator: the C ABI of include/drnmf_reverb.h and its argument validation
on a handle bound to no device, the host-side draws and helpers, the checks ops.MixBank / fit_mixtures /
from_mixtures make of their reverb arguments before they touch a device, and the yardstick: the float32
restatement of the header's chain against the fp64 reference, from which the bound of tests/test_gpu_reverb.py is
taken, and the mutants of the reference, which must all miss it (no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import reverb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drnmf_reverb.h")
NAMES = {"drnmf_reverb_forward"}

BOUND = R.BOUND           # pinned there with its derivation; this file measures what it is derived from


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return set(re.findall(r"\b(drnmf_[a-z0-9_]+)\s*\(", src))


def test_reverb_header_is_plain_c_and_matches_the_binding(capi, tmp_path):
    declared = _declared()
    assert declared == NAMES
    assert declared == set(capi.REVERB_SIGNATURES)
    assert capi.REVERB_SIGNATURES in capi.SIGNATURE_TABLES
    for t in dir(capi):
        if t.endswith("SIGNATURES") and t != "REVERB_SIGNATURES":
            assert not (declared & set(getattr(capi, t))), t
    for hdr in os.listdir(os.path.join(ROOT, "include")):
        if hdr != "drnmf_reverb.h":
            assert "drnmf_reverb_" not in open(os.path.join(ROOT, "include", hdr)).read(), hdr
    L = capi.lib()
    for name in sorted(declared):
        fn = getattr(L, name)                 # exported ...
        assert fn.argtypes == capi.REVERB_SIGNATURES[name][1]       # ... and bound by _capi.lib()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in declared:
        assert name in doc, name
    from drnmf_amd import ops
    assert (ops.REVERB_TILE, ops.REVERB_CHUNK) == (capi.REVERB_TILE, capi.REVERB_CHUNK)
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "no C compiler"
    src = tmp_path / "reverb_header_check.c"
    src.write_text('#include "drnmf_reverb.h"\ntypedef void (*fn_t)(void);\nstatic const fn_t refs[] = {\n' +
                   "".join("    (fn_t)%s,\n" % n for n in sorted(declared)) +
                   "};\nint main(void) { return refs[0] != 0 && DRNMF_REVERB_TILE == %d && DRNMF_REVERB_CHUNK == %d "
                   "? 0 : 1; }\n" % (capi.REVERB_TILE, capi.REVERB_CHUNK))
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(src)], check=True)
    # the definition is in the header word for word
    text = re.sub(r"\s*\n \*\s*", " ", open(HDR).read())
    for piece in ("acc = fmaf(h[t], s[.], acc), starting from +0.0f, in ascending t",
                  "Terms whose sample lies outside the signal are skipped",
                  "exactly e[k] when E == L",
                  "both outputs are the speech as float32, bit for bit, and no RIR is read",
                  "Every element of both outputs is written and none outside them",
                  "No atomics.  No workgroup waits for another"):
        assert piece in text, piece


def test_reverb_entry_point_validates_without_a_gpu(capi):
    """On a drnmf_create_unbound handle: a NULL handle, every bad shape and every required NULL pointer return
    DRNMF_ERR_INVALID_ARG, the latter two with their messages and the shape before the pointers; a fully valid
    call, with or without the optional tables, stops only at the missing device."""
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)          # never dereferenced: the call stops before any launch

        def forward(handle=h, n_sig=3, ss=1001, ls=fake, i16=0, sp=fake, n_rir=2, sr=777, lr=fake, rirs=fake, idx=fake,
                    delay=fake, early_n=fake, wet=fake, early=fake):
            return L.drnmf_reverb_forward(handle, n_sig, ss, ls, i16, sp, n_rir, sr, lr, rirs, idx, delay, early_n, wet,
                                          early, None)

        who = b"reverb_forward"
        assert forward(handle=None) == -1
        # the size-0 cases among them: no signals, no RIRs, rows of no samples
        for kw in (dict(n_sig=0), dict(n_sig=-2), dict(ss=0), dict(ss=-7), dict(n_rir=0), dict(n_rir=-1), dict(sr=0),
                   dict(sr=-3), dict(sr=2 ** 30 + 1), dict(ss=2 ** 40 + 1), dict(i16=2), dict(i16=-1)):
            assert forward(**kw) == -1, kw
            msg = L.drnmf_last_error(h)
            assert who in msg and b"bad shape" in msg, (kw, msg)
        pointers = ("ls", "sp", "lr", "rirs", "idx", "wet")
        for name in pointers:
            assert forward(**{name: None}) == -1, name
            assert who in L.drnmf_last_error(h) and b"NULL" in L.drnmf_last_error(h)
            # precedence: a bad shape is reported before a NULL pointer
            assert forward(n_sig=0, **{name: None}) == -1
            assert b"bad shape" in L.drnmf_last_error(h), name
        for kw in (dict(), dict(delay=None), dict(early_n=None), dict(early=None), dict(delay=None, early_n=None, early=None),
                   dict(i16=1), dict(sr=2 ** 30), dict(n_sig=70000)):
            rc = forward(**kw)
            assert rc not in (0, -1, -2, -4) and who in L.drnmf_last_error(h) and \
                b"no device" in L.drnmf_last_error(h), (kw, rc)
        # ... and a NULL pointer before the missing device
        assert forward(wet=None) == -1
    finally:
        L.drnmf_destroy(h)


def test_rir_draw_is_a_pure_function_and_leaves_the_mix_draw_alone(capi):
    from drnmf_amd import ops
    n, n_rir = 400, 7
    a = ops.rir_draw(n, n_rir, seed=3, epoch=2)
    assert a.dtype == np.int32 and a.shape == (n,) and np.array_equal(a, ops.rir_draw(n, n_rir, seed=3, epoch=2))
    assert a.min() == 0 and a.max() == n_rir - 1 and len(set(a.tolist())) == n_rir        # reverb_prob = 1: none dry
    for other in (dict(seed=3, epoch=3), dict(seed=4, epoch=2)):
        assert not np.array_equal(a, ops.rir_draw(n, n_rir, **other)), other
    # the recipe, written out; the number of dry utterances is what it gives
    for p in (0.0, 0.25, 0.5, 1.0):
        rs = np.random.RandomState((3 * 998244353 + 2 * 7919 + 0x52495221) % 2 ** 32)
        want = rs.randint(0, n_rir, n).astype(np.int32)
        dry = rs.random_sample(n) >= p
        want[dry] = -1
        got = ops.rir_draw(n, n_rir, seed=3, epoch=2, reverb_prob=p)
        assert np.array_equal(got, want), p
        assert int((got == -1).sum()) == int(dry.sum()), p
        assert np.array_equal(got[got >= 0], a[got >= 0])            # the RIR of a wet utterance does not depend on p
    assert (ops.rir_draw(n, n_rir, reverb_prob=0.0) == -1).all()
    assert 0.15 * n < (ops.rir_draw(n, n_rir, reverb_prob=0.25) >= 0).sum() < 0.35 * n
    # salted differently from mix_draw: not its noise indices
    assert not np.array_equal(a, ops.mix_draw(n, np.full(n_rir, 9))[0])
    for bad in (dict(n=0), dict(n_rir=0), dict(reverb_prob=-0.1), dict(reverb_prob=1.5), dict(reverb_prob=float("nan"))):
        with pytest.raises(ValueError, match="rir_draw"):
            ops.rir_draw(**dict(dict(n=5, n_rir=3), **bad))

    # a bank's draw: MixBank.draw without a device (the method reads n, len_noise and n_rir only)
    class Bank(object):
        draw = ops.MixBank.draw
        _check_draw = ops.MixBank._check_draw

        def __init__(self, n_rir):
            self.n, self.n_noise, self.n_rir = 50, 3, n_rir
            self.len_noise = np.array([5, 4096, 30000], dtype=np.int64)

    dry, wet = Bank(0), Bank(4)
    for kw in (dict(seed=1, epoch=0), dict(seed=1, epoch=5, snr_db=(-3.0, 3.0)), dict(seed=2, snr_choices=[0.0, 5.0])):
        d3, d4 = dry.draw(**kw), wet.draw(**kw)
        assert len(d3) == 3 and len(d4) == 4
        for u, v in zip(d3, d4):
            assert u.dtype == v.dtype and np.array_equal(u, v)
        assert np.array_equal(d4[3], ops.rir_draw(50, 4, seed=kw["seed"], epoch=kw.get("epoch", 0)))
        assert all(np.array_equal(u, v) for u, v in zip(d4, wet.draw(**kw)))
        half = wet.draw(reverb_prob=0.5, **kw)
        assert all(np.array_equal(u, v) for u, v in zip(half[:3], d3)) and (half[3] == -1).any()
        # each bank accepts exactly its own arity
        assert len(dry._check_draw(d3)) == 3 and len(wet._check_draw(d4)) == 4
        for bank, d in ((dry, d4), (wet, d3)):
            with pytest.raises(ValueError, match="a draw is"):
                bank._check_draw(d)
    d4 = wet.draw(seed=1)
    for bad in (d4[3].astype(np.int64), d4[3][:-1], np.full(50, 4, np.int32), np.full(50, -2, np.int32)):
        with pytest.raises(ValueError, match="rir_index"):
            wet._check_draw(d4[:3] + (bad,))


def test_rir_delays_take_the_first_maximum(capi):
    from drnmf_amd import ops
    f = lambda *v: np.array(v, dtype=np.float32)
    rirs = [f(1), f(0, 0.5, -0.5, 0.2), f(0.1, -0.9, 0.9, 0.9), f(0, 0, 0), f(-2, 1, 2)]
    d = ops.rir_delays(rirs)
    assert d.dtype == np.int32 and d.tolist() == [0, 1, 1, 0, 0]
    for bad in ([], [f()], [np.zeros(3)], [np.zeros((2, 2), np.float32)], [f(1, float("nan"))]):
        with pytest.raises(ValueError, match="rir_delays"):
            ops.rir_delays(bad)


def test_early_counts_are_capped_before_they_are_added(capi):
    from drnmf_amd import ops
    d = np.array([0, 9, 2 ** 31 - 2], dtype=np.int32)
    got = ops.rir_early_counts(d, 5.0, 16000)
    assert got.dtype == np.int32 and got.tolist() == [81, 90, 2 ** 31 - 1]
    assert ops.rir_early_counts(d, 0.0, 16000).tolist() == [1, 10, 2 ** 31 - 1]
    assert ops.rir_early_counts(d[:2], 0.03, 16000).tolist() == [1, 10]              # round(0.48) = 0
    # a huge finite span: capped, no OverflowError
    for ms in (1e12, 1e300, 1.7e308):
        assert ops.rir_early_counts(d, ms, 16000).tolist() == [2 ** 31 - 1] * 3, ms
    for ms in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="rir_early_counts"):
            ops.rir_early_counts(d, ms, 16000)


def test_synthetic_rirs_are_reproducible_and_finite(capi):
    from drnmf_amd import ops
    a = ops.synthetic_rirs(6, fs=8000, rt60=(0.1, 0.3), seed=4)
    b = ops.synthetic_rirs(6, fs=8000, rt60=(0.1, 0.3), seed=4)
    assert len(a) == 6
    for u, v in zip(a, b):
        assert u.dtype == np.float32 and u.ndim == 1 and np.array_equal(u, v) and np.isfinite(u).all()
        assert 800 <= len(u) <= 2400 and u[0] == 1.0 and np.argmax(np.abs(u)) == 0
        # -60 dB at the end: the last tenth lies below 10^-2.7 of the tail's scale (5 sigma)
        assert np.abs(u[-len(u) // 10:]).max() <= 5 * ops.SYNTHETIC_RIR_TAIL * 10 ** -2.7
        assert np.abs(u[1:len(u) // 10]).max() > 0.5 * ops.SYNTHETIC_RIR_TAIL
    assert len(set(len(u) for u in a)) > 1
    assert not np.array_equal(a[0][:800], ops.synthetic_rirs(6, fs=8000, rt60=(0.1, 0.3), seed=5)[0][:800])
    assert ops.rir_delays(a).tolist() == [0] * 6
    one = ops.synthetic_rirs(1)[0]
    assert 0.2 * 16000 <= len(one) <= 0.8 * 16000
    for bad in (dict(n=0), dict(rt60=(0.0, 0.5)), dict(rt60=(0.5, 0.2)), dict(fs=0)):
        with pytest.raises(ValueError, match="synthetic_rirs"):
            ops.synthetic_rirs(**dict(dict(n=2), **bad))


def test_reverb_arguments_are_refused_before_the_device_is_touched(capi):
    """These run on a machine without a GPU: the checks come before the first allocation."""
    from drnmf_amd import layers, ops
    a = np.zeros(1000, np.int16)
    h = np.array([1.0, 0.5], np.float32)
    params = dict(r=4, sparsity=0.1, cf='ed', max_iter=2, conv_eps=0., random_seed=1)
    bad_rirs = ([], [h, np.zeros(0, np.float32)], [h.astype(np.float64)], [np.zeros((2, 2), np.float32)],
                [np.array([1.0, np.inf], np.float32)], [np.array([np.nan], np.float32)])
    bad_kw = [dict(rirs=r) for r in bad_rirs] + \
        [dict(rirs=[h], target_speech='wet'), dict(rirs=[h], target_speech='dry', align=False),
         dict(rirs=[h], early_ms=-1.0), dict(rirs=[h], early_ms=float("nan")), dict(rirs=[h], fs=0),
         dict(target_speech='anechoic')]

    class Fake(layers._SequenceModel):
        def __init__(self):
            self.mask_value = -1.0

        def _device(self):
            return "cuda:0"

        def _input_width(self):
            return 257

    for kw in bad_kw:
        with pytest.raises(ValueError, match="MixBank"):
            ops.MixBank([a], [a], **kw)
        with pytest.raises(ValueError, match="from_mixtures"):
            layers.SparseNMFModel.from_mixtures([a], [a], params, N=64, hop=16, **kw)
        with pytest.raises(ValueError, match="fit_mixtures"):
            Fake().fit_mixtures([a], [a], **kw)
    # the sides are still checked first, as without RIRs
    with pytest.raises(ValueError, match="clean"):
        ops.MixBank([], [a], rirs=[])
    # reverb_forward's own checks need no device either
    import torch
    sp, ln = torch.zeros(2, 10), torch.zeros(2, dtype=torch.int64)
    rr, lr, idx = torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    tab = torch.zeros(3, dtype=torch.int32)
    for args, kw, what in (((sp.double(), ln, rr, lr, idx), {}, "speech"), ((sp, ln, rr.double(), lr, idx), {}, "rirs"),
                           ((sp, ln, rr[:, :0], lr, idx), {}, "rirs"), ((sp, ln.int(), rr, lr, idx), {}, "len_s"),
                           ((sp, ln, rr, lr[:2], idx), {}, "len_r"), ((sp, ln, rr, lr, idx.long()), {}, "rir_index"),
                           ((sp, ln, rr, lr, idx), dict(delay=tab[:2]), "delay"),
                           ((sp, ln, rr, lr, idx), dict(n_early=tab.long()), "n_early"),
                           ((sp, ln, rr, lr, idx), dict(out=torch.zeros(2, 9)), "out"),
                           ((sp, ln, rr, lr, idx), dict(early_out=torch.zeros(2, 10, dtype=torch.float64)), "early_out")):
        with pytest.raises(ValueError, match=what):
            ops.reverb_forward(*args, **kw)


def _outputs(b, fn, **kw):
    return lambda i: fn(b["speech"][i], b["rirs"][b["idx"][i]], b["delay"][b["idx"][i]], b["n_early"][b["idx"][i]], **kw)


def test_the_yardstick_holds_a_quarter_of_the_bound_and_every_mutant_misses_it(capi):
    T, C = capi.REVERB_TILE, capi.REVERB_CHUNK
    batches = [R.batch(n_sig, int16, T, C) for n_sig in (1, 5, 70) for int16 in (True, False)]
    big = batches[-1]
    assert set(big["lens"].tolist()) == set(R.speech_lens(T)) and len(set(big["idx"].tolist())) == 21
    assert set(len(h) for h in big["rirs"]) == set(R.rir_lens(T, C)) and max(len(h) for h in big["rirs"]) > big["lens"].max()
    yardstick = max(R.worst_err(b, _outputs(b, R.reverb_one_f32)) for b in batches)
    print("yardstick (float32 chain against fp64): %.3g; bound %.3g" % (yardstick, BOUND))
    assert 0 < yardstick <= BOUND / 4, yardstick
    assert BOUND == 2e-5 and 8 * yardstick <= BOUND < 16 * yardstick      # the pinned literal is the rule's, not a looser one
    misses = {}
    for m in R.MUTANTS:
        misses[m] = max(R.worst_err(b, _outputs(b, R.reverb_one, mutant=m, tile=T, chunk=C)) for b in batches) / BOUND
        assert misses[m] > 1, (m, misses[m])
    weakest = min(misses, key=misses.get)
    print("weakest mutant: %s misses the bound by a factor of %.3g" % (weakest, misses[weakest]))
    # measured: window_last_zero, by 5.0e4 (an error of 1.0 of the largest sample: a unit tap dropped)
    assert misses[weakest] > 100, (weakest, misses[weakest])
    # the reference itself: no mutation, no error; the degenerate rows are the speech
    assert all(R.worst_err(b, _outputs(b, R.reverb_one)) == 0.0 for b in batches)
    s = big["speech"][5]
    for h in (None, np.zeros(0, np.float32)):
        wet, early = R.reverb_one(s, h)
        assert np.array_equal(wet, R.as_float(s)) and np.array_equal(early, wet)
        wet, early = R.reverb_one_f32(s, h)
        assert np.array_equal(wet, R.as_float(s).astype(np.float32)) and np.array_equal(early, wet)
    # and against a plain double loop on a small case, delay and early part included
    rng = np.random.default_rng(2)
    s, h = rng.standard_normal(9).astype(np.float32), rng.standard_normal(5).astype(np.float32)
    for d, E in ((0, 5), (2, 3), (4, 0), (9, 9), (None, None)):
        dd, EE = R.clamp(d, E, 5)
        want = np.zeros((2, 9))
        for k in range(9):
            for t in range(5):
                if 0 <= k + dd - t < 9:
                    want[0 if t < EE else 1, k] += float(h[t]) * float(s[k + dd - t])
        wet, early = R.reverb_one(s, h, d, E)
        assert np.allclose(wet, want[0] + want[1], rtol=0, atol=1e-14) and np.allclose(early, want[0], rtol=0, atol=1e-14)
        w32, e32 = R.reverb_one_f32(s, h, d, E)
        assert np.allclose(w32, wet, rtol=0, atol=1e-5) and np.allclose(e32, early, rtol=0, atol=1e-5)
