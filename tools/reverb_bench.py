"""A fresh draw of reverberant training mixtures on the device (ops.MixBank with RIRs) against the same bank without
RIRs and against the route it replaces, scipy.signal.fftconvolve on the host.  One JSON line, appended to
profiles/reverb_bench.jsonl.

    python tools/reverb_bench.py [--utts 512] [--noises 32] [--rirs 32] [--taps 8192] [--reps 15] [--host-reps 3]
                                 [--variant tree]

Workload: tools/mix_bench.py's (--utts utterances of 2 to 6 s at 16 kHz, lengths drawn with seed 0, --noises
recordings of 60 s, int16 noise-like samples on both sides, SNRs uniform in [-6, 9] dB, N = 512, hop = 128, maxlen =
500) plus --rirs RIRs of --taps taps (Gaussian noise under a 60 dB decay behind a unit direct path), every utterance
reverberated.  After one warm-up of each route the device routes alternate --reps times in one process; every timed
call ends in a synchronise and a new epoch's draw is made for every repeat outside the timed part.
  bank_rir_s      bank.tensors(draw, out=(x, y, w)) with RIRs: four index tables up, the reverb launch, the mixer
                  (which now also computes the wet speech's energy), the pair kernels
  bank_dry_s      the same call on a bank without RIRs
  reverb_us       device events around ops.reverb_forward alone (wet only, as target_speech='reverberant' runs it),
                  median of --reps; reverb_early_us: with the early output as well
  reverb_tflops   2 flop per (output, tap the definition counts) over reverb_us: outputs whose sample lies before
                  the signal's start or behind its end are not counted
  host_fft_s      scipy.signal.fftconvolve(clean float32, rir)[:n] for every utterance, one at a time, median of
                  --host-reps: what a user ran before, without the upload that would follow it
  variant         --variant as given: `tree` for the kernel as committed, another name for a line measured with a
                  kernel under trial, so that the lines of the file can be told apart
  wet_max_rel     max |device wet - fftconvolve| / max |fftconvolve| over the utterances of the last host repeat
JSON goes to stdout, nothing else does.
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

N_FFT, HOP, MAXLEN, FS = 512, 128, 500, 16000
DEV = "cuda:0"


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    del out
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=512)
    ap.add_argument("--noises", type=int, default=32)
    ap.add_argument("--rirs", type=int, default=32)
    ap.add_argument("--taps", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--variant", default="tree")
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    from scipy.signal import fftconvolve
    if not torch.cuda.is_available():
        raise SystemExit("reverb_bench needs a GPU")
    rng = np.random.default_rng(0)
    lengths = rng.integers(2 * FS, 6 * FS + 1, size=a.utts).astype(np.int64)
    clean = [rng.integers(-3000, 3000, size=int(l)).astype(np.int16) for l in lengths]
    noise = [rng.integers(-3000, 3000, size=60 * FS).astype(np.int16) for _ in range(a.noises)]
    rirs = []
    for _ in range(a.rirs):
        h = 0.05 * rng.standard_normal(a.taps) * 10.0 ** (-3.0 * np.arange(a.taps) / a.taps)
        h[0] = 1.0
        rirs.append(h.astype(np.float32))
    wet_bank = ops.MixBank(clean, noise, rirs=rirs, device=DEV)
    dry_bank = ops.MixBank(clean, noise, device=DEV)
    kw = dict(N=N_FFT, hop=HOP, maxlen=MAXLEN)
    out_w = wet_bank.tensors(wet_bank.draw(seed=1, epoch=0), **kw)              # warm-up of both routes
    out_d = dry_bank.tensors(dry_bank.draw(seed=1, epoch=0), **kw)
    t = dict(rir=[], dry=[])
    for rep in range(a.reps):
        dw, dd = wet_bank.draw(seed=1, epoch=1 + rep), dry_bank.draw(seed=1, epoch=1 + rep)
        t["rir"].append(timed(lambda: wet_bank.tensors(dw, out=out_w, **kw)))
        t["dry"].append(timed(lambda: dry_bank.tensors(dd, out=out_d, **kw)))
    ev = dict(wet=[], early=[])
    early = torch.empty_like(wet_bank.wet)
    for rep in range(a.reps):
        idx = torch.from_numpy(wet_bank.draw(seed=1, epoch=100 + rep)[3]).to(DEV)
        for key, eo in (("wet", None), ("early", early)):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.reverb_forward(wet_bank.clean, wet_bank.len_clean_dev, wet_bank.rirs, wet_bank.len_rir_dev, idx,
                               delay=wet_bank.rir_delay, n_early=wet_bank.rir_n_early, out=wet_bank.wet, early_out=eo)
            e1.record()
            torch.cuda.synchronize()
            ev[key].append(e0.elapsed_time(e1) * 1e3)
    # the host route, and the device's wet speech against it
    draw = wet_bank.draw(seed=1, epoch=100 + a.reps - 1)
    dev_wet = wet_bank._download(wet_bank.wet)
    clean32 = [v.astype(np.float32) / np.float32(32768.0) for v in clean]
    host = []
    for rep in range(a.host_reps):
        t0 = time.perf_counter()
        ref = [fftconvolve(s, rirs[j])[:len(s)] for s, j in zip(clean32, draw[3])]
        host.append(time.perf_counter() - t0)
    rel = max(float(np.max(np.abs(d - r)) / np.max(np.abs(r))) for d, r in zip(dev_wet, ref))
    # the terms the definition counts: output k of n meets taps 0 .. min(L - 1, k) (delay 0 here)
    L = a.taps
    terms = 0
    for n in lengths.tolist():
        m = min(n, L)
        terms += m * (m + 1) // 2 + (n - m) * L
    us = float(np.median(ev["wet"]))
    res = dict(tool="reverb_bench", utts=a.utts, noises=a.noises, rirs=a.rirs, taps=a.taps, fs=FS,
               lengths="uniform 2-6 s (seed 0)", N=N_FFT, hop=HOP, maxlen=MAXLEN, reps=a.reps, host_reps=a.host_reps,
               total_s=int(lengths.sum()) / FS, device=torch.cuda.get_device_name(0),
               tile=ops.REVERB_TILE, chunk=ops.REVERB_CHUNK,
               bank_rir_s=round(float(np.median(t["rir"])), 5), bank_dry_s=round(float(np.median(t["dry"])), 5),
               bank_rir_s_all=[round(v, 5) for v in t["rir"]], bank_dry_s_all=[round(v, 5) for v in t["dry"]],
               reverb_us=round(us, 1), reverb_us_all=[round(v, 1) for v in ev["wet"]],
               reverb_early_us=round(float(np.median(ev["early"])), 1),
               reverb_flop=2 * terms, reverb_tflops=round(2 * terms / us / 1e6, 2),
               host_fft_s=round(float(np.median(host)), 3), host_fft_s_all=[round(v, 3) for v in host],
               wet_max_rel=rel, variant=a.variant)
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "reverb_bench.jsonl"), "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
