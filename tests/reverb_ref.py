"""The definition of include/drnmf_reverb.h in numpy, one signal at a time: what the device-side reverberator is
checked against.

    wet, early = reverb_one(speech, h_or_None, delay, n_early)            fp64
    wet, early = reverb_one_f32(speech, h_or_None, delay, n_early)        the same ascending chains in float32

speech: 1-D int16 (a sample is v / 32768, exact in float32) or float32; h: 1-D float32.  The fp64 form adds the
exact products in fp64 (the order of an fp64 sum is 1e-16 relative and plays no part against float32); the float32
form is the yardstick of tests/test_reverb_host.py: the header's chain acc = acc + h[t] * s[.] in ascending t with
the product and the sum each rounded to float32, where the device rounds once (fmaf).

`mutant=` names one deliberate mistake of the fp64 form (MUTANTS): the checks of the device must be tight enough
to catch each of them on the case list `batch()` below, which both test files share."""
import numpy as np

# max |device - fp64| / max |fp64| per signal and output.  DESIGN.md 4.4's rule: the device may order nothing
# differently inside a chain, but its fmaf rounds once where the float32 restatement below rounds twice, so the bound
# is the restatement's own error over the case list (2.46e-6, measured by tests/test_reverb_host.py, which also holds
# it to a quarter of the bound) times 8 = 1.97e-5, rounded up to one digit.
BOUND = 2e-5

MUTANTS = ("last_tap_dropped", "first_tap_dropped", "delay_plus_one", "delay_minus_one", "early_plus_one",
           "early_minus_one", "chunk_tap_doubled", "window_last_zero")


def as_float(v):
    """The float32 sample values as fp64."""
    v = np.asarray(v)
    if v.dtype == np.int16:
        return v.astype(np.float64) / 32768.0
    assert v.dtype == np.float32, v.dtype
    return v.astype(np.float64)


def clamp(delay, n_early, L):
    """(d, E) of the header: d into [0, L-1], E into [0, L]; None: 0 / all taps."""
    d = 0 if delay is None else min(max(int(delay), 0), L - 1)
    E = L if n_early is None else min(max(int(n_early), 0), L)
    return d, E


def _part(s, h, t_a, t_b, d, n):
    """sum_{t in [t_a, t_b)} h[t] s[k + d - t], k < n, s = 0 outside [0, n); d may be any integer."""
    if t_b <= t_a:
        return np.zeros(n)
    c = np.convolve(s, h[t_a:t_b])                     # c[m] = sum_t h[t_a + t] s[m - t], m < n + (t_b - t_a) - 1
    out = np.zeros(n)
    m = np.arange(n) + d - t_a
    ok = (m >= 0) & (m < c.shape[0])
    out[ok] = c[m[ok]]
    return out


def reverb_one(speech, h, delay=None, n_early=None, mutant=None, tile=None, chunk=None):
    """(wet, early) of one signal in fp64; h None or empty: both are the speech.  mutant: one of MUTANTS (tile and
    chunk, the kernel's constants, are needed by the last two)."""
    s = as_float(speech)
    n = s.shape[0]
    if h is None or len(h) == 0:
        return s.copy(), s.copy()
    h = np.asarray(h)
    assert h.dtype == np.float32 and h.ndim == 1
    h = h.astype(np.float64)
    L = h.shape[0]
    d, E = clamp(delay, n_early, L)
    assert mutant is None or mutant in MUTANTS, mutant
    if mutant == "last_tap_dropped":
        h[L - 1] = 0.0
    elif mutant == "first_tap_dropped":
        h[0] = 0.0
    elif mutant == "delay_plus_one":
        d += 1
    elif mutant == "delay_minus_one":
        d -= 1
    elif mutant == "early_plus_one":
        E = min(E + 1, L)
    elif mutant == "early_minus_one":
        E = max(E - 1, 0)
    elif mutant == "chunk_tap_doubled" and L > chunk:
        h[chunk] *= 2.0
    early = _part(s, h, 0, E, d, n)
    late = _part(s, h, E, L, d, n)
    if mutant == "window_last_zero":
        # the last position of a (tile, chunk) window is the sample the tile's last output meets at the chunk's
        # first tap
        for k in range(tile - 1, n, tile):
            for t0 in range(0, L, chunk):
                m = k + d - t0
                if 0 <= m < n:
                    (early if t0 < E else late)[k] -= h[t0] * s[m]
    return early + late, early


def reverb_one_f32(speech, h, delay=None, n_early=None):
    """(wet, early) as float32 by the header's chains with two roundings per term; terms outside the signal are
    skipped."""
    s = as_float(speech).astype(np.float32)
    n = s.shape[0]
    if h is None or len(h) == 0:
        return s.copy(), s.copy()
    h = np.asarray(h, dtype=np.float32)
    L = h.shape[0]
    d, E = clamp(delay, n_early, L)
    acc = [np.zeros(n, np.float32), np.zeros(n, np.float32)]
    for t in range(L):
        # k + d - t in [0, n)  <=>  k in [t - d, n + t - d)
        k_a, k_b = max(0, t - d), min(n, n + t - d)
        if k_a < k_b:
            a = acc[0 if t < E else 1]
            a[k_a:k_b] = a[k_a:k_b] + h[t] * s[k_a + d - t:k_b + d - t]
    return (acc[0] + acc[1] if E < L else acc[0].copy()), acc[0]


# ---- the case list both test files share ------------------------------------------------------------------
def speech_lens(T):
    return [1, 2, T - 1, T, T + 1, 2 * T + 5]


def rir_lens(T, C):
    return [1, 2, C - 1, C, C + 1, 2 * C + 3, 2 * T + 5 + 395]        # the last: longer than the longest signal


def rir_bank(T, C, seed=7):
    """21 RIRs: each of the seven lengths with each kind of delay (0, L - 1, an interior one); the early counts
    (0, 1, C - 1, C, L, L + 9) cycle at another period, so every one meets several lengths and delays.  Taps:
    Gaussian of standard deviation 0.3 under a decay of 20 dB over the RIR, h[delay] = 1: the last tap matters.
    Returns (list of float32 arrays, delay int32 [21], n_early int32 [21])."""
    rng = np.random.default_rng(seed)
    lens = rir_lens(T, C)
    hs, delay, n_early = [], [], []
    for r in range(21):
        L = lens[r % 7]
        d = (0, L - 1, L // 3)[r // 7]
        E = (0, 1, C - 1, C, L, L + 9)[r % 6]
        h = 0.3 * rng.standard_normal(L) * 10.0 ** (-np.arange(L) / float(L))
        h[d] = 1.0
        hs.append(h.astype(np.float32))
        delay.append(d)
        n_early.append(E)
    return hs, np.array(delay, dtype=np.int32), np.array(n_early, dtype=np.int32)


def signal(rng, n, scale, int16):
    v = scale * rng.standard_normal(n)
    if not int16:
        return v.astype(np.float32)
    v = np.clip(np.round(v * 32768.0), -32768, 32767).astype(np.int16)
    v[v == 0] = 1
    return v


_batches = {}


def batch(n_sig, int16, T, C):
    """n_sig in (1, 5, 70) signals over rir_bank: signal q of the 70 has length speech_lens[q % 6] and RIR
    (5 q + q // 21) % 21; the batches of 1 and 5 are signals 41.. and 20.. of the same rule.  Built once per key with
    its fp64 reference and never modified."""
    key = (n_sig, bool(int16), T, C)
    if key not in _batches:
        hs, delay, n_early = rir_bank(T, C)
        q0 = {1: 41, 5: 20, 70: 0}[n_sig]
        rng = np.random.default_rng(100 * n_sig + int(int16))
        lens = [speech_lens(T)[(q0 + i) % 6] for i in range(n_sig)]
        idx = np.array([(5 * (q0 + i) + (q0 + i) // 21) % 21 for i in range(n_sig)], dtype=np.int32)
        speech = [signal(rng, n, (0.05, 0.2, 0.5)[i % 3], int16) for i, n in enumerate(lens)]
        ref = [reverb_one(speech[i], hs[idx[i]], delay[idx[i]], n_early[idx[i]]) for i in range(n_sig)]
        _batches[key] = dict(speech=speech, lens=np.array(lens, dtype=np.int64), idx=idx, rirs=hs, delay=delay,
                             n_early=n_early, ref=ref)
    return _batches[key]


def rel_err(got, ref):
    """max |got - ref| / max |ref| of one output of one signal (0 / 0 = 0)."""
    den = float(np.max(np.abs(ref)))
    num = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)))
    return 0.0 if num == 0.0 else num / den if den > 0 else float("inf")


def worst_err(b, outputs):
    """The largest rel_err over a batch's signals and both outputs; outputs(i) -> (wet, early) of signal i."""
    worst = 0.0
    for i, ref in enumerate(b["ref"]):
        got = outputs(i)
        worst = max(worst, rel_err(got[0], ref[0]), rel_err(got[1], ref[1]))
    return worst
