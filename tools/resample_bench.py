"""Rate conversion on the device (ops.resample, ops.MixBank(noise_fs=)) against the route it replaces,
scipy.signal.resample_poly on the host plus the upload of its result.  One JSON line, appended to
profiles/resample_bench.jsonl (--out).

    python tools/resample_bench.py [--recs 512] [--seconds 4] [--reps 15] [--host-reps 1] [--out FILE]

Workload: --recs recordings of --seconds s of int16 noise at 48000 and at 44100 Hz, converted to 16000 Hz.  Per rate,
after a warm-up:
  kernel_us       device events around a loop of --reps ops.resample calls on samples already in device memory
                  (out= given), divided by --reps: the launch alone
  bytes           what the definition moves: 2 bytes per input sample, 4 per output
  tb_per_s        bytes over kernel_us; hbm_share: over 8 TB/s, the HBM's peak (the kernel should be bandwidth-bound)
  call_s          ops.resample on the host list, ending in a synchronise: the pinned upload and the launch, median
  host_s          scipy.signal.resample_poly(x float32, p, q, window=h / p) for every recording, one at a time, plus
                  the upload of the result (torch.from_numpy(...).to(device), synchronised), median of --host-reps
  max_abs_err     max |device - scipy| over the first 8 recordings, samples scaled to [-1, 1)
bank_s: building ops.MixBank(clean, noise48, noise_fs=48000) (--recs clean recordings of --seconds s at 16000 Hz),
ending in a synchronise, median of 5; bank_host_s: resample_poly on the noise side, then ops.MixBank on the result.
JSON goes to stdout, nothing else does.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

FS = 16000
DEV = "cuda:0"
HBM_PEAK = 8.0e12


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    del out
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recs", type=int, default=512)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.jsonl"))
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    import resample_ref as R
    from scipy.signal import resample_poly
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs a GPU")
    rng = np.random.default_rng(0)
    res = dict(tool="resample_bench", recs=a.recs, seconds=a.seconds, fs_out=FS, reps=a.reps, host_reps=a.host_reps,
               device=torch.cuda.get_device_name(0), rates={})
    keep48 = None
    for fs_in in (48000, 44100):
        n = int(round(a.seconds * fs_in))
        wavs = [rng.integers(-3000, 3000, size=n).astype(np.int16) for _ in range(a.recs)]
        p, q = ops.resample_rate(fs_in, FS)
        h = R.filter_taps(p, q)
        pcm = torch.from_numpy(np.stack(wavs)).to(DEV)
        lens = np.full(a.recs, n, dtype=np.int64)
        y, n_out = ops.resample(pcm, fs_in, FS, lengths=lens)                       # warm-up: taps, code object
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            ops.resample(pcm, fs_in, FS, lengths=lens, out=y)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.reps
        ops.resample(wavs, fs_in, FS, device=DEV)
        call = [timed(lambda: ops.resample(wavs, fs_in, FS, device=DEV)) for _ in range(a.reps)]
        host, ref = [], None
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            ref = [resample_poly(w.astype(np.float32) / np.float32(32768.0), p, q, window=h / p) for w in wavs]
            up = torch.from_numpy(np.stack(ref).astype(np.float32)).to(DEV)
            torch.cuda.synchronize()
            host.append(time.perf_counter() - t0)
            del up
        yh = y[:8].cpu().numpy()
        err = max(float(np.abs(yh[i, :int(n_out[i])] - ref[i]).max()) for i in range(min(8, a.recs)))
        nbytes = 2 * a.recs * n + 4 * int(n_out.sum())
        res["rates"][str(fs_in)] = dict(
            p=p, q=q, taps=len(h), tile=ops.resample_tile(fs_in, FS), samples_in=a.recs * n, samples_out=int(n_out.sum()),
            kernel_us=round(us, 1), bytes=nbytes, tb_per_s=round(nbytes / us / 1e6, 3),
            hbm_share=round(nbytes / (us * 1e-6) / HBM_PEAK, 3), call_s=round(float(np.median(call)), 5),
            call_s_all=[round(v, 5) for v in call], host_s=round(float(np.median(host)), 3),
            host_s_all=[round(v, 3) for v in host], max_abs_err=err)
        if fs_in == 48000:
            keep48 = wavs
        del pcm, y
    clean = [rng.integers(-3000, 3000, size=int(a.seconds * FS)).astype(np.int16) for _ in range(a.recs)]
    ops.MixBank(clean, keep48, noise_fs=48000, device=DEV)
    bank = [timed(lambda: ops.MixBank(clean, keep48, noise_fs=48000, device=DEV)) for _ in range(5)]
    h = R.filter_taps(1, 3)
    bank_host = []
    for _ in range(a.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        low = [resample_poly(w.astype(np.float32) / np.float32(32768.0), 1, 3, window=h).astype(np.float32)
               for w in keep48]
        ops.MixBank(clean, low, device=DEV)
        torch.cuda.synchronize()
        bank_host.append(time.perf_counter() - t0)
    res.update(bank_s=round(float(np.median(bank)), 4), bank_s_all=[round(v, 4) for v in bank],
               bank_host_s=round(float(np.median(bank_host)), 3), bank_host_s_all=[round(v, 3) for v in bank_host])
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
