"""fp64 numpy restatement of the STOI criterion and its exact gradient -- the contract of include/drnmf_stoi_loss.h.
The forward is tests/stoi_ref.py stage by stage; the backward walks the same stages in reverse.  No scipy, no GPU.

loss = -STOI(x, y) for x the reference and y the estimate.  The silence decision and the compaction index depend on
x only, so the loss is differentiable in y except on the clip ties (alpha Y = c X) and at zero envelopes:
  segments    d = <x^, y^> of the centred, normalised X and Y' = min(alpha Y, c X), alpha = sqrt(Sx / Sy):
                  dd/dY' = (x^ - d y^) / ||Y' - mean|| =: g,
                  dd/dY_t = alpha u_t g_t - (alpha / Sy) Y_t sum_s u_s g_s Y_s,   u_t = [alpha Y_t <= c X_t];
              a segment-band with Sy == 0 (scored 1 through fmin's NaN rule) contributes zero gradient;
  envelopes   Y = sqrt(sum_band |Z_k|^2): G_k = gY Z_k / Y on the band's bins (0 where Y == 0), and the frame's
              sample gradient is w[n] Re sum_k G_k e^{+2 pi i k n / 512}, n < 256;
  compaction  band frame i covers compacted samples 128 i .. 128 i + 255; kept frame c at source start s_c gives
              g_y10k[s_c + n] += w[n] g_ys[128 c + n];
  resampling  g_est[k] = sum_m g_y10k[m] h[q m + (L-1)/2 - p k] (skipped at 10 kHz).
A row is COUNTED iff its forward STOI is finite: fewer than 30 band frames or a NaN from a zero-variance band give
loss 0, gradient 0, counted False.
"""
import numpy as np

import stoi_ref as SR


def resample_vjp(g10k, n, fs):
    """Transpose of stoi_ref.resample for an input of n samples at fs: g10k [ceil(n p / q)] -> [n]."""
    g10k = np.asarray(g10k, dtype=np.float64)
    if int(fs) == SR.FS:
        return g10k.copy()
    h, p, q, half = SR.resample_filter(fs)
    L = len(h)
    ny = len(g10k)
    k = np.arange(n, dtype=np.int64)[:, None]
    m = (p * k - half + q - 1) // q + np.arange(L // q + 2, dtype=np.int64)[None, :]    # every m with h index <= L-1
    t = q * m + half - p * k
    ok = (t >= 0) & (t < L) & (m >= 0) & (m < ny)
    return np.where(ok, g10k[np.clip(m, 0, max(ny - 1, 0))] * h[np.clip(t, 0, L - 1)], 0.0).sum(axis=1)


def segment_grads(X, Y):
    """(d [S, 15], gY [nf, 15]): the segment scores of stoi_ref.segment_scores and the gradient of their SUM with
    respect to the envelopes Y (X, Y [nf, 15])."""
    nf = X.shape[0]
    S = max(nf - SR.N_SEG + 1, 0)
    d = np.zeros((S, SR.J))
    gY = np.zeros_like(Y, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for m in range(S):
            xs, ys = X[m:m + SR.N_SEG], Y[m:m + SR.N_SEG]
            sx, sy = (xs ** 2).sum(0), (ys ** 2).sum(0)
            alpha = np.sqrt(sx / sy)
            ay, cx = ys * alpha, xs * SR.CLIP
            yp = np.fmin(ay, cx)
            u = ay <= cx                                   # (NaN compares False: fmin then took c X)
            xc, yc = xs - xs.mean(0), yp - yp.mean(0)
            nx, ny = np.sqrt((xc ** 2).sum(0)), np.sqrt((yc ** 2).sum(0))
            xh, yh = xc / nx, yc / ny
            d[m] = (xh * yh).sum(0)
            g = (xh - d[m] * yh) / ny
            c2 = (np.where(u, g * ys, 0.0)).sum(0) * alpha / sy
            contrib = np.where(u, alpha * g, 0.0) - c2 * ys
            gY[m:m + SR.N_SEG] += np.where(sy > 0.0, contrib, 0.0)
    return d, gY


def envelope_vjp(ys, gY):
    """Gradient with respect to the compacted signal ys of sum(gY * band_envelopes(ys))."""
    w = SR.hanning(SR.N_FRAME)
    st = SR.frame_starts(len(ys))
    out = np.zeros(len(ys))
    n = np.arange(SR.N_FRAME)
    for i, s in enumerate(st):
        Z = np.fft.fft(ys[s:s + SR.N_FRAME] * w, SR.NFFT)
        G = np.zeros(SR.NFFT, dtype=np.complex128)
        for j, (lo, hi) in enumerate(SR.BANDS):
            env = np.sqrt((np.abs(Z[lo:hi]) ** 2).sum())
            if env > 0.0:
                G[lo:hi] = gY[i, j] * Z[lo:hi] / env
        # Re sum_k G_k e^{+2 pi i k n / 512} = 512 Re ifft(G)
        out[s:s + SR.N_FRAME] += w * (SR.NFFT * np.fft.ifft(G)).real[n]
    return out


def compaction_vjp(g_ys, keep, n10k):
    """Transpose of stoi_ref.remove_silent_frames' overlap-add of y for the decision `keep`."""
    w = SR.hanning(SR.N_FRAME)
    st = SR.frame_starts(n10k)
    out = np.zeros(n10k)
    c = 0
    for j, s in enumerate(st):
        if keep[j]:
            out[s:s + SR.N_FRAME] += w * g_ys[SR.HOP * c:SR.HOP * c + SR.N_FRAME]
            c += 1
    return out


def stoi_loss(x, y, fs, device_roundings=False):
    """(loss, counted, g): loss = -STOI(x, y) and g = d loss / d y [len(y)] in fp64; an uncounted row gives
    (0.0, False, zeros).  device_roundings=True applies the two float32 roundings of csrc/stoi.hip's pipeline -- the
    band envelopes the forward stores and the segment stage reads back, and g as it is stored -- and nothing else:
    what the device's result differs by from the fp64 one if the rest of its arithmetic is exact."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    x10, y10 = SR.resample(x, fs), SR.resample(y, fs)
    xs, ys, keep = SR.remove_silent_frames(x10, y10)
    X, Y = SR.band_envelopes(xs), SR.band_envelopes(ys)
    if device_roundings:
        X, Y = X.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64)
    d, gY = segment_grads(X, Y)
    with np.errstate(invalid="ignore"):
        val = float(d.mean()) if d.size else float("nan")
    if not np.isfinite(val):
        return 0.0, False, np.zeros(n)
    g_ys = envelope_vjp(ys, -gY / d.size)
    g10 = compaction_vjp(g_ys, keep, len(y10))
    g = resample_vjp(g10, n, fs)
    return -val, True, g.astype(np.float32).astype(np.float64) if device_roundings else g


def rel_err(a, b):
    """max |a - b| / max |b|: the max-norm relative error wave_loss_ref.rel_err uses."""
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))) /
                 max(float(np.max(np.abs(b))), 1e-300))


# ---- the issue's table of cases: (seed, n, fs, snr, gaps) ---------------------------------------------------------
CASES = [(0, 4500, 10000, 5.0, True), (1, 12000, 16000, 0.0, True), (2, 7300, 16000, -5.0, False),
         (3, 6000, 8000, 5.0, True), (4, 5000, 16000, 5.0, True), (6, 6554, 16000, 0.0, False),
         (6, 6553, 16000, 0.0, False), (6, 4097, 10000, 0.0, False), (6, 4096, 10000, 0.0, False)]
EXPECTED = {(0, 4500): -0.78644, (1, 12000): -0.79140, (2, 7300): -0.60573, (3, 6000): -0.82706}


def pair(seed, n, fs, snr, gaps):
    """(x, y) float32: speech_like and its noisy copy from one default_rng(seed), both rounded to float32."""
    rng = np.random.default_rng(seed)
    x = SR.speech_like(rng, n, fs, gaps=gaps)
    y = SR.add_noise(rng, x, snr)
    return x.astype(np.float32), y.astype(np.float32)


def stretch_pair():
    """Seed 1 with y[3000:9000] = 0: segments whose estimate is digitally silent (Sy == 0) beside ordinary ones."""
    x, y = pair(1, 12000, 16000, 0.0, True)
    y = y.copy()
    y[3000:9000] = 0.0
    return x, y
