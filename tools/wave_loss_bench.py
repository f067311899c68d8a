"""What a waveform criterion costs: one training step through the inverse STFT (model.train_on_wavs) against the
spectral step on the same rows (model.train_on_batch), and the transposed inverse in one kernel
(ops.istft_ragged_vjp) against its composition from the forward transform.  One JSON line, appended to
profiles/wave_loss_bench.jsonl (--out: another file).

    python tools/wave_loss_bench.py [--reps 9] [--inner 5] [--out FILE]

Workload: B = 8 and 32 recordings of 63 360 samples (3.96 s at 16 kHz: T = 500 frames at N = 512, hop = 128, F =
257), noise-like float32 on both sides; the recurrent cell at r = 100, K = 2 and the LSTM baseline at H = 256, K = 2.
Every timed window is --inner calls and ends in a synchronise; the two routes of a comparison alternate --reps times
in one process after a warm-up of each.  Reported per comparison: the median per call and every repeat's value.
  (a) wavs_step_s    model.train_on_wavs (loss 'si_sdr'): upload, STFT, training forward, head, cropped inverse, loss,
                     transposed inverse, head backward, BPTT, Adam
      wavs_dev_s     the same step from waveforms already on the device (loss_and_grads_cot on a prepared bank +
                     apply_gradients): what fit_waveform pays per step
      batch_step_s   model.train_on_batch on x, y, w of the same recordings (ops.wavs_to_tensors, on the device)
  (b) vjp_s          ops.istft_ragged_vjp
      composed_s     ops.stft_ragged of g, then (re * G.re + im * G.im) * c in torch elementwise passes
      vjp_max_diff   largest difference of the two results over max|result| (they are the same quantity)
Nothing here is asserted.  JSON goes to stdout, nothing else does.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_FFT, HOP, T, FS = 512, 128, 500, 16000
F = N_FFT // 2 + 1
NSAMPL = (T - N_FFT // HOP - 1) * HOP
DEV = "cuda:0"


def window(fn, inner):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    del out
    return (time.perf_counter() - t) / inner


def alternate(routes, reps, inner):
    for fn in routes.values():
        window(fn, 1)
    t = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            t[k].append(window(fn, inner))
    return {k: dict(median=round(float(np.median(v)), 6), all=[round(x, 6) for x in v]) for k, v in t.items()}


def build(family):
    from drnmf_amd import layers
    if family == "snmf":
        rng = np.random.default_rng(0)
        W = rng.random((F, 200)) ** 4
        W = (W / np.sqrt((W * W).sum(0, keepdims=True))).astype(np.float32)
        np.random.seed(0)
        m = layers.build_unfolded_snmf(dict(input_dim=F, hidden_dim=200, output_dim=F, mask_value=-1., maxseq=T,
                                            K_layers=2, W=W, alph=50.0, lam1=0.3,
                                            params_untied=["log_D", "log_alph"],
                                            params_trainable=["log_D", "log_alph"]))
    else:
        m = layers.build_lstm(dict(mask_value=-1.0, maxseq=T, input_dim=F, output_dim=F, K_layers=2, hidden_dim=256),
                              device=torch.device(DEV))
    return m.compile(lr=1e-5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_loss_bench.jsonl"))
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("wave_loss_bench needs a GPU")
    rng = np.random.default_rng(0)
    res = dict(tool="wave_loss_bench", N=N_FFT, hop=HOP, T=T, F=F, nsampl=NSAMPL, reps=a.reps, inner=a.inner,
               device=torch.cuda.get_device_name(0), steps={}, vjp={})
    for B in (8, 32):
        clean = [(0.1 * rng.standard_normal(NSAMPL)).astype(np.float32) for _ in range(B)]
        noisy = [c + (0.05 * rng.standard_normal(NSAMPL)).astype(np.float32) for c in clean]
        for family in ("snmf", "lstm"):
            m = build(family)
            x, y, w = ops.wavs_to_tensors(noisy, clean, N=N_FFT, hop=HOP, maxlen=T, mask_value=-1.0, device=DEV)
            assert tuple(x.shape) == (B, T, F), tuple(x.shape)
            bank = m._wave_bank(noisy, clean, N_FFT, HOP, None, "wave_loss_bench")
            rows = np.arange(B)

            def dev_step():
                xb, cot = m._wave_batch(bank, rows, N_FFT, HOP, "si_sdr")
                return m.apply_gradients(m.loss_and_grads_cot(xb, cot))
            r = alternate(dict(wavs_step_s=lambda: m.train_on_wavs(noisy, clean, N=N_FFT, hop=HOP),
                               wavs_dev_s=dev_step,
                               batch_step_s=lambda: m.train_on_batch(x, y, w)), a.reps, a.inner)
            r["ratio_dev_over_batch"] = round(r["wavs_dev_s"]["median"] / r["batch_step_s"]["median"], 3)
            res["steps"]["%s_B%d" % (family, B)] = r
            del m
        # (b) the transposed inverse against its composition
        lens = [NSAMPL] * B
        pcm = torch.from_numpy(np.stack(noisy)).to(DEV)
        _, re, im, _ = ops.stft_ragged(pcm, lens, N=N_FFT, hop=HOP)
        g = torch.randn((B, NSAMPL), device=DEV)
        c = torch.full((F,), 2.0, device=DEV)
        c[0] = c[-1] = 1.0
        c = c * (2.0 * HOP / N_FFT / N_FFT)
        out = torch.empty_like(re)

        def composed():
            _, gr, gi, _ = ops.stft_ragged(g, lens, N=N_FFT, hop=HOP)
            return (re * gr + im * gi) * c
        r = alternate(dict(vjp_s=lambda: ops.istft_ragged_vjp(g, re, im, lens, N_FFT, HOP, crop=True, out=out),
                           composed_s=composed), a.reps, 4 * a.inner)
        d = composed()
        r["vjp_max_diff"] = float((out - d).abs().max() / d.abs().max())
        r["ratio_vjp_over_composed"] = round(r["vjp_s"]["median"] / r["composed_s"]["median"], 3)
        res["vjp"]["B%d" % B] = r
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
