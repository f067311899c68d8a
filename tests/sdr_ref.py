"""References for the stages of the device SDR (csrc/sdr.hip), each independent of the code under test and of one
another: exact integer correlations, Levinson-Durbin in mpmath, the projection in long double with its running
error bound, and an exact Toeplitz residual.  numpy and mpmath only; no GPU.

Why the correlation can be compared with a tolerance of ZERO.  The test signals are "what a 16-bit file holds":
integers v, |v| <= 20000, handed to the device as float32(v / 32768), which is exact.  A product of two samples is
v w / 2^30 with |v w| <= 4e8, and over a row of at most 48000 samples every partial sum of such products, over any
subset and in any order, is an integer multiple of 2^-30 below 4e8 * 48000 = 1.92e13 < 2^53 in units of 2^-30.  So
every fp64 product, fma and addition the device can perform on the way to r[a] and d[a] is exact, whatever the
tiling, the split into spans or the order of the partial sums, and the result must equal the integer sum / 2^30 bit
for bit."""
import numpy as np
import mpmath

PEAK = 20000
SCALE = 32768.0
U = 2.0 ** -53


def int16_values(x, peak=PEAK):
    """x scaled to the given peak and rounded: (integers as int64, the float32 the device is given)."""
    v = np.round(np.asarray(x, np.float64) / np.max(np.abs(x)) * peak).astype(np.int64)
    return v, (v / SCALE).astype(np.float32)


def as_int16_values(x32):
    """The integers behind a float32 array of v / 32768 (asserts that it is one)."""
    v = np.round(np.asarray(x32, np.float64) * SCALE)
    assert np.array_equal((v / SCALE).astype(np.float32), np.asarray(x32, np.float32))
    return v.astype(np.int64)


def exact_corr(est_i, ref_i, flen):
    """r[a] = sum_n ref[n] ref[n-a], d[a] = sum_n est[n] ref[n-a], a < flen, as int64 sums of integer products.
    The device's fp64 values must equal these / 2^30 bitwise (module docstring); the precondition is asserted."""
    est_i = np.asarray(est_i)
    ref_i = np.asarray(ref_i)
    assert est_i.dtype == np.int64 and ref_i.dtype == np.int64 and est_i.shape == ref_i.shape and est_i.ndim == 1
    n = ref_i.shape[0]
    peak = max(int(np.max(np.abs(est_i), initial=0)), int(np.max(np.abs(ref_i), initial=0)))
    assert peak * peak * max(n, 1) < 2 ** 53, "every partial sum must stay below 2^53 (peak %d, %d samples)" % (peak, n)
    r = np.zeros(flen, np.int64)
    d = np.zeros(flen, np.int64)
    for a in range(min(flen, n)):
        r[a] = np.dot(ref_i[a:], ref_i[:n - a])
        d[a] = np.dot(est_i[a:], ref_i[:n - a])
    return r, d


def exact_corr_f64(est_i, ref_i, flen):
    """exact_corr / 2^30 as float64: exact, since the integers are below 2^53."""
    r, d = exact_corr(est_i, ref_i, flen)
    return r.astype(np.float64) / 2.0 ** 30, d.astype(np.float64) / 2.0 ** 30


def toeplitz(r):
    n = r.shape[0]
    return r[np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])]


def levinson_mp(r, d, dps=60):
    """Solve Toeplitz(r) c = d by Levinson-Durbin in mpmath at `dps` digits (Python floats convert exactly).
    Returns a list of mpf.  About a second at n = 512, tens of seconds at 2048."""
    with mpmath.workdps(dps):
        r = [mpmath.mpf(float(v)) for v in r]
        d = [mpmath.mpf(float(v)) for v in d]
        n = len(r)
        fdot = mpmath.fdot
        E = r[0]
        x = [d[0] / E]
        if n == 1:
            return x
        alpha = -r[1] / E
        y = [alpha]
        for k in range(1, n):
            E = E * (1 - alpha * alpha)
            rk = r[k:0:-1]                                   # r[k - i], i < k
            mu = (d[k] - fdot(rk, x)) / E
            x = [x[i] + mu * y[k - 1 - i] for i in range(k)]
            x.append(mu)
            if k < n - 1:
                alpha = -(r[k + 1] + fdot(rk, y)) / E
                y = [y[i] + alpha * y[k - 1 - i] for i in range(k)]
                y.append(alpha)
        return x


def mp_to_f64(c):
    return np.array([float(v) for v in c], np.float64)


def mp_to_ld(c):
    """mpf list -> np.longdouble, keeping the bits below float64 (hi + lo)."""
    hi = np.array([float(v) for v in c], np.float64)
    lo = np.array([float(v - mpmath.mpf(float(v))) for v in c], np.float64)
    return hi.astype(np.longdouble) + lo.astype(np.longdouble)


def residual_mp(r, d, c, dps=60):
    """||T c - d||_inf / ||d||_inf in mpmath for an mpf solution c.  Used only to validate levinson_mp itself (the
    issue's "< 1e-40 relative"); solver comparisons use scaled_residual below."""
    with mpmath.workdps(dps):
        n = len(c)
        rm = [mpmath.mpf(float(v)) for v in r]
        full = rm[:0:-1] + rm                                # full[n - 1 + k] = r[|k|]
        worst = mpmath.mpf(0)
        for i in range(n):
            row = full[n - 1 - i:2 * n - 1 - i]
            worst = max(worst, abs(mpmath.fdot(row, c) - mpmath.mpf(float(d[i]))))
        return worst / max(abs(mpmath.mpf(float(v))) for v in d)


_SHIFT = 1100                                                # 2^-1074 is the smallest float64 step


def _exact_ints(x):
    out = np.empty(len(x), dtype=object)
    for i, v in enumerate(x):
        num, den = float(v).as_integer_ratio()
        out[i] = (num << _SHIFT) // den                      # exact: den is a power of two <= 2^1074
    return out


def scaled_residual(r, d, c):
    """||T c - d||_inf / (||T||_inf ||c||_inf + ||d||_inf) for float64 r, d, c, with T c - d evaluated EXACTLY
    (every float64 is an integer multiple of 2^-1100; Python integers) and rounded once at the end."""
    r = np.asarray(r, np.float64)
    d = np.asarray(d, np.float64)
    c = np.asarray(c, np.float64)
    n = c.shape[0]
    assert r.shape[0] >= n and d.shape[0] >= n and np.all(np.isfinite(c))
    r, d = r[:n], d[:n]
    ri, di, ci = _exact_ints(r), _exact_ints(d), _exact_ints(c)
    full = np.concatenate([ri[:0:-1], ri])
    worst = 0
    for i in range(n):
        v = np.dot(full[n - 1 - i:2 * n - 1 - i], ci) - (di[i] << _SHIFT)
        worst = max(worst, abs(v))
    with mpmath.workdps(40):
        res = float(mpmath.ldexp(mpmath.mpf(worst), -2 * _SHIFT))
    ra = np.abs(r)
    full_a = np.concatenate([ra[:0:-1], ra])
    t_inf = max(float(np.sum(full_a[n - 1 - i:2 * n - 1 - i])) for i in range(n))
    return res / (t_inf * float(np.max(np.abs(c))) + float(np.max(np.abs(d))))


def project_ld(est, ref, c):
    """The BSS Eval projection for one row in np.longdouble: s = conv(ref, c) over len + flen - 1 samples,
    num = sum s^2, den = sum (est - s)^2 (est zero-padded).  Returns (num, den, B_num, B_den) with the running-error
    terms B_num = sum_n (sum_a |c_a| |ref[n-a]|)^2 and B_den = sum_n (|est[n]| + sum_a |c_a| |ref[n-a]|)^2."""
    ld = np.longdouble
    est = np.asarray(est).astype(ld)
    ref = np.asarray(ref).astype(ld)
    c = np.asarray(c).astype(ld)
    n, flen = ref.shape[0], c.shape[0]
    if n == 0:
        return ld(0), ld(0), 0.0, 0.0
    s = np.convolve(ref, c)
    assert s.dtype == ld and s.shape[0] == n + flen - 1
    e = np.concatenate([est, np.zeros(flen - 1, ld)])
    num = np.sum(s * s)
    den = np.sum((e - s) * (e - s))
    sa = np.convolve(np.abs(ref).astype(np.float64), np.abs(c).astype(np.float64)) * (1.0 + 1e-12)
    ea = np.abs(e).astype(np.float64)
    return num, den, float(np.sum(sa * sa)), float(np.sum((ea + sa) * (ea + sa)))


def gamma(k):
    return k * U / (1.0 - k * U)


def projection_bound(n, flen, B):
    """Forward bound on |computed - exact| of num (or den) for ANY fp64 evaluation that forms each s[n] by a dot
    product of flen terms and sums the L = n + flen - 1 squares in a tree or chain of depth <= 2 log2 L + 3
    (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 and 4.2): a computed s[n] is off by at most
    gamma_flen * sum_a |c_a ref[n-a]|, its square by twice that relatively, and each of the additions adds one
    rounding per level, so the sum is off by at most (2 gamma_flen + gamma_depth) B <= 2 gamma_k B with
    k = flen + ceil(log2 L) + 2: gamma_k B for the dot products plus the same for the final sums."""
    L = n + flen - 1
    k = flen + int(np.ceil(np.log2(max(L, 1)))) + 2
    return 2.0 * gamma(k) * B


def db(num, den):
    return float(10.0 * np.log10(np.longdouble(num) / np.longdouble(den)))
