"""STOI over a batch sized like the CHiME2 test set: one JSON line.

    python tools/stoi_bench.py [--pairs 1980] [--fs 16000] [--reps 5] [--oracle-pairs 3] [--extended]

The real utterance lengths are not part of this project, so they are drawn (seed 0) uniformly from 2 to 12 s
(mean 7 s).  Rows are slices of a bank of 8 speech-like 12 s references (tests/stoi_ref.py: speech_like);
estimates add white noise at an SNR drawn from {-6, -3, 0, 3, 6, 9} dB.  Fields:
  gpu_ms          median of --reps timed ops.stoi calls on the whole batch (CUDA events), after one warm-up
                  call; device tensors in, the [n_pairs] score out; resampling included
  utt_per_s       pairs / gpu_ms
  oracle_s_per_pair  the fp64 numpy restatement (tests/stoi_ref.py) on the CPU, mean over --oracle-pairs rows
  max_abs_err     max |GPU - oracle| over those rows
--extended times three calls in one session, each as gpu_ms is timed, and adds:
  estoi_ms        ops.estoi alone (the envelopes, then ESTOI's segment and mean kernels)
  pair_ms         ops.stoi_ext: STOI and ESTOI from one set of envelopes (drnmf_stoi_ext)
  pair_over_stoi  pair_ms / gpu_ms
  estoi_max_abs_err  max |GPU - tests/estoi_ref.py| over the oracle rows; pair_bits_equal: the pair call returns
                  the bits of the two single calls
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1980)
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle-pairs", type=int, default=3)
    ap.add_argument("--extended", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    import stoi_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("stoi_bench needs a GPU")
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

    def timed(fn):
        out = fn()                                            # warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = fn()
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1))
        return out, times

    out, times = timed(lambda: ops.stoi(est, ref, fs=fs, lengths=lengths))
    gpu_ms = float(np.median(times))
    got = out.cpu().numpy()
    ext = {}
    if a.extended:
        import estoi_ref as ER
        out_e, t_e = timed(lambda: ops.estoi(est, ref, fs=fs, lengths=lengths))
        (pair_s, pair_e), t_p = timed(lambda: ops.stoi_ext(est, ref, fs=fs, lengths=lengths))
        got_e = out_e.cpu().numpy()
    rows = np.argsort(lengths)[:: max(1, n // max(a.oracle_pairs, 1))][:a.oracle_pairs]
    E, X = est.cpu().numpy(), ref.cpu().numpy()
    errs, t_or = [], 0.0
    for i in rows:
        t = time.perf_counter()
        want = R.stoi(X[i, :lengths[i]].astype(np.float64), E[i, :lengths[i]].astype(np.float64), fs)
        t_or += time.perf_counter() - t
        errs.append(abs(float(got[i]) - want))
    if a.extended:
        errs_e = [abs(float(got_e[i]) - ER.estoi(X[i, :lengths[i]].astype(np.float64),
                                                 E[i, :lengths[i]].astype(np.float64), fs)) for i in rows]
        ext = dict(estoi_ms=round(float(np.median(t_e)), 3), estoi_ms_all=[round(t, 3) for t in t_e],
                   pair_ms=round(float(np.median(t_p)), 3), pair_ms_all=[round(t, 3) for t in t_p],
                   pair_over_stoi=round(float(np.median(t_p)) / gpu_ms, 3),
                   estoi_max_abs_err=float(max(errs_e)) if errs_e else None, mean_estoi=float(np.nanmean(got_e)),
                   estoi_nan_rows=int(np.isnan(got_e).sum()),
                   pair_bits_equal=bool(pair_s.cpu().numpy().tobytes() == got.tobytes() and
                                        pair_e.cpu().numpy().tobytes() == got_e.tobytes()))
    print(json.dumps(dict(
        tool="stoi_bench", pairs=n, fs=fs, lengths="uniform 2-12 s (seed 0)", total_s=float(lengths.sum()) / fs,
        gpu_ms=round(gpu_ms, 3), gpu_ms_all=[round(t, 3) for t in times], utt_per_s=round(n / gpu_ms * 1e3, 1),
        oracle_s_per_pair=round(t_or / max(len(rows), 1), 3), oracle_pairs=int(len(rows)),
        max_abs_err=float(max(errs)) if errs else None, mean_stoi=float(np.nanmean(got)),
        device=torch.cuda.get_device_name(0), **ext)))


if __name__ == "__main__":
    main()
