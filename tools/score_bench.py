"""SDR (and the whole compute_scores row) over a batch sized like the CHiME2 test set: one JSON line.

    python tools/score_bench.py [--pairs 1980] [--fs 16000] [--reps 5] [--host-only | --no-host] [--out FILE]

The set is tools/stoi_bench.py's: lengths drawn (seed 0) uniformly from 2 to 12 s, rows sliced from a bank of 8
speech-like 12 s references (tests/stoi_ref.py: speech_like), estimates = reference + white noise at an SNR from
{-6, -3, 0, 3, 6, 9} dB, zero behind each row's length.  Every figure is wall-clock milliseconds around a call
that ends in a stream synchronisation (the host solver works on the host, so device events would miss it):
the median of --reps calls after one warm-up call, and all of them (`*_all`).  Fields:
  sdr_host_ms        ops.sdr_db(est, ref): correlations and projection on the device, Toeplitz systems on the host
  sdr_host_solve_share   share of that spent inside np.linalg.solve (timed by wrapping it)
  stoi_ms            ops.stoi on the same set, for scale
  sdr_device_ms      ops.sdr_db(est, ref, lengths=, solver="device")
  scores_host_ms / scores_device_ms   ops.compute_scores(...) / ops.compute_scores(..., sdr_solver="device")
  max_abs_db_diff    largest |dB| difference between the two solvers over the set
  info_counts        counts of the solve's info word (0 = solved)
--host-only calls nothing but ops.sdr_db(est, ref) and ops.stoi as they exist before the device solver (it runs on
a checkout that lacks it); --no-host skips the host-solver calls (profiling runs).  The line goes to stdout and is
appended to --out (default profiles/score_bench.jsonl)."""
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


def _timed(fn, reps, what):
    fn()                                                        # warm-up
    torch.cuda.synchronize()
    times, res = [], None
    for k in range(reps):
        t = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
        print("%s rep %d: %.3f ms" % (what, k, times[-1]), file=sys.stderr, flush=True)
    return res, round(float(np.median(times)), 3), [round(t, 3) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1980)
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.jsonl"))
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    import stoi_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("score_bench needs a GPU")
    fs, n = a.fs, a.pairs
    rng = np.random.default_rng(0)
    lengths = rng.integers(2 * fs, 12 * fs + 1, size=n).astype(np.int64)
    width = int(lengths.max())
    bank = np.stack([R.speech_like(np.random.default_rng(100 + i), 12 * fs, fs) for i in range(8)])
    bank = torch.from_numpy(bank.astype(np.float32)).cuda()
    pick = rng.integers(0, 8, size=n)
    snr = rng.choice([-6.0, -3.0, 0.0, 3.0, 6.0, 9.0], size=n)
    dev = torch.device("cuda:0")
    ref = bank[torch.from_numpy(pick).to(dev), :width].contiguous()
    col = torch.arange(width, device=dev)[None, :]
    valid = col < torch.from_numpy(lengths).to(dev)[:, None]
    ref = torch.where(valid, ref, torch.zeros_like(ref))
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    noise = torch.randn(ref.shape, generator=g, device=dev) * valid
    p_ref = (ref.double() ** 2).sum(1) / (noise.double() ** 2).sum(1)
    scale = torch.sqrt(p_ref / torch.from_numpy(10.0 ** (snr / 10.0)).to(dev)).float()
    est = (ref + noise * scale[:, None]).contiguous()
    del noise, valid, col

    out = dict(tool="score_bench", pairs=n, fs=fs, lengths="uniform 2-12 s (seed 0)",
               total_s=float(lengths.sum()) / fs, padded_over_ragged=round(float(n * width) / float(lengths.sum()), 3),
               reps=a.reps, device=torch.cuda.get_device_name(0))
    host_db = None
    if not a.no_host:
        solve_s = [0.0]
        real_solve = np.linalg.solve

        def timed_solve(*args, **kw):
            t = time.perf_counter()
            try:
                return real_solve(*args, **kw)
            finally:
                solve_s[0] += time.perf_counter() - t
        np.linalg.solve = timed_solve
        try:
            host_db, ms, ms_all = _timed(lambda: ops.sdr_db(est, ref), a.reps, "sdr host")
        finally:
            np.linalg.solve = real_solve
        out.update(sdr_host_ms=ms, sdr_host_ms_all=ms_all,
                   sdr_host_solve_share=round(solve_s[0] * 1e3 / (a.reps + 1) / float(np.mean(ms_all)), 3))
        host_db = host_db.cpu().numpy()
        out.update(mean_sdr_host_db=float(np.mean(host_db)))
    _, ms, ms_all = _timed(lambda: ops.stoi(est, ref, fs=fs, lengths=lengths), a.reps, "stoi")
    out.update(stoi_ms=ms, stoi_ms_all=ms_all)
    if not a.host_only:
        ld = torch.from_numpy(lengths).to(dev)
        parts, ms, ms_all = _timed(lambda: ops.sdr_db(est, ref, lengths=ld, solver="device", return_parts=True),
                                   a.reps, "sdr device")
        dev_db, info = parts[0].cpu().numpy(), parts[3].cpu().numpy()
        vals, counts = np.unique(info, return_counts=True)
        out.update(sdr_device_ms=ms, sdr_device_ms_all=ms_all, mean_sdr_device_db=float(np.mean(dev_db)),
                   info_counts={str(int(v)): int(c) for v, c in zip(vals, counts)})
        if host_db is not None:
            out.update(max_abs_db_diff=float(np.max(np.abs(dev_db.astype(np.float64) - host_db))))
        if not a.no_host:
            _, ms, ms_all = _timed(lambda: ops.compute_scores(est, ref, fs, lengths, lengths), a.reps, "scores host")
            out.update(scores_host_ms=ms, scores_host_ms_all=ms_all)
        _, ms, ms_all = _timed(lambda: ops.compute_scores(est, ref, fs, lengths, lengths, sdr_solver="device"),
                               a.reps, "scores device")
        out.update(scores_device_ms=ms, scores_device_ms_all=ms_all)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
