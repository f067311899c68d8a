"""What the STOI criterion costs: ops.stoi_loss (the score and its gradient) against ops.stoi (the score alone) on
the same pairs, and one training step under loss='stoi' against the step under 'si_sdr' on the same batch.  One JSON
line, appended to profiles/stoi_loss_bench.jsonl (--out: another file).

    python tools/stoi_loss_bench.py [--reps 9] [--inner 5] [--out FILE]

Workload: 8 recordings of 4 s at 16 kHz (64 000 samples; after resampling 40 000 samples at 10 kHz, 311 silence-
detector frames), speech-like float32 (tests/stoi_ref.py's generator) against noisy copies at 5 dB; for the steps the
recurrent cell at r = 100, K = 2 and the LSTM baseline at H = 256, K = 2, N = 512, hop = 128.  Every timed window is
--inner calls and ends in a synchronise; the two routes of a comparison alternate --reps times in one process after a
warm-up of each.  Reported per comparison: the median per call and every repeat's value.
  (a) stoi_s         ops.stoi (workspace and output allocated per call, as a caller sees it)
      stoi_loss_s    ops.stoi_loss
  (b) stoi_step_s    the step of fit_waveform(loss='stoi') from a resident bank (loss_and_grads_cot + apply_gradients)
      si_sdr_step_s  the same with loss='si_sdr'
Nothing here is asserted.  JSON goes to stdout, nothing else does.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from wave_loss_bench import alternate, build, N_FFT, HOP, DEV  # noqa: E402

FS, B, NSAMPL = 16000, 8, 64000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stoi_loss_bench.jsonl"))
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    import stoi_ref as SR
    if not torch.cuda.is_available():
        raise SystemExit("stoi_loss_bench needs a GPU")
    rng = np.random.default_rng(0)
    clean = [SR.speech_like(rng, NSAMPL, FS).astype(np.float32) for _ in range(B)]
    noisy = [SR.add_noise(rng, c.astype(np.float64), 5.0).astype(np.float32) for c in clean]
    res = dict(tool="stoi_loss_bench", fs=FS, B=B, nsampl=NSAMPL, N=N_FFT, hop=HOP, reps=a.reps, inner=a.inner,
               device=torch.cuda.get_device_name(0), steps={})
    est, ref, lens = torch.from_numpy(np.stack(noisy)).to(DEV), torch.from_numpy(np.stack(clean)).to(DEV), [NSAMPL] * B
    r = alternate(dict(stoi_s=lambda: ops.stoi(est, ref, fs=FS, lengths=lens),
                       stoi_loss_s=lambda: ops.stoi_loss(est, ref, lens, fs=FS)), a.reps, 4 * a.inner)
    loss, counted, _, _ = ops.stoi_loss(est, ref, lens, fs=FS)
    r["counted"] = int(counted.sum())
    r["mean_stoi"] = round(-float(loss.sum()) / max(r["counted"], 1), 6)
    r["ratio_loss_over_stoi"] = round(r["stoi_loss_s"]["median"] / r["stoi_s"]["median"], 3)
    res["ops"] = r
    rows = np.arange(B)
    for family in ("snmf", "lstm"):
        m = build(family)
        bank = m._wave_bank(noisy, clean, N_FFT, HOP, None, "stoi_loss_bench")

        def step(kind):
            xb, cot = m._wave_batch(bank, rows, N_FFT, HOP, kind, FS)
            return m.apply_gradients(m.loss_and_grads_cot(xb, cot))
        r = alternate(dict(stoi_step_s=lambda: step("stoi"), si_sdr_step_s=lambda: step("si_sdr")), a.reps, a.inner)
        r["ratio_stoi_over_si_sdr"] = round(r["stoi_step_s"]["median"] / r["si_sdr_step_s"]["median"], 3)
        res["steps"]["%s_B%d" % (family, B)] = r
        del m
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
