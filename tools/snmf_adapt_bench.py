"""Wall time of the noise-adaptive sparse-NMF baseline against the only way to do the job without it.

    python tools/snmf_adapt_bench.py [--iters 200] [--batches 1,16,250] [--frames 500] [--reps 5]
                                     [--out profiles/snmf_adapt_bench.jsonl]

At the shipped dictionary size (F = 257, N = 200, the 100 speech atoms fixed), T frames per row and the reference's
200 iterations, for B = 1, 16 and 250 rows: median milliseconds of
  loop     a per-row Python loop over ops.SnmfTrainer with the speech half frozen (w_update_mask) and the same
           initial H: drnmf_snmf_train_step's device-wide launches on one row's frames at a time.  Measured in front
           of (loop_before) and behind (loop_after) the new path, to show drift inside the session.
  adapt    ops.snmf_adapt_forward on the whole batch
  fixed    ops.snmf_mask_forward on the same input: what the baseline costs without adaptation
Every configuration is warmed once and timed with device events; one JSON line per (B, path) is appended to --out,
the adapt line with the largest difference of its dictionaries from the loop's.  Nothing is asserted about speed."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F, N, N0, SPARSITY = 257, 200, 100, 0.1


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batches", default="1,16,250")
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snmf_adapt_bench.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    if not torch.cuda.is_available():
        raise RuntimeError("snmf_adapt_bench needs a GPU: a time taken anywhere else says nothing")
    from drnmf_amd import ops
    dev = "cuda:0"
    rng = np.random.RandomState(0)
    W = rng.rand(F, N) + 0.05
    Wn = torch.from_numpy((W / np.sqrt((W * W).sum(0))).astype(np.float32)).to(dev)
    hn = torch.from_numpy(rng.rand(N).astype(np.float32)).to(dev)
    frozen = torch.from_numpy((np.arange(N) >= N0).astype(np.uint8)).to(dev)
    T = a.frames
    lines = []
    for B in [int(v) for v in a.batches.split(",")]:
        g = torch.Generator(device=dev).manual_seed(B)
        x = torch.rand((B, T, F), generator=g, device=dev) ** 2 + 1e-3
        H0 = hn[None].expand(T, N).contiguous()
        ws = ops.snmf_adapt_workspace(B, T, F, N, N0, dev)
        got = {}

        def loop():
            last = None
            for b in range(B):
                tr = ops.SnmfTrainer(x[b], Wn, H0)
                for _ in range(a.iters):
                    tr.step(SPARSITY, frozen, True)
                last = tr.W
            got["loop_W_last"] = last

        def adapt():
            got["adapt"] = ops.snmf_adapt_forward(x, Wn, hn, SPARSITY, a.iters, N0, mask_value=-1.0, workspace=ws,
                                                  return_dictionaries=True)

        def fixed():
            ops.snmf_mask_forward(x, Wn, hn, SPARSITY, a.iters, mask_value=-1.0)

        for name, fn in (("loop_before", loop), ("adapt", adapt), ("fixed", fixed), ("loop_after", loop)):
            timed(fn, 1)                             # warm-up: code objects, workspaces
            ms = timed(fn, a.reps)
            line = dict(tool="snmf_adapt_bench", path=name, B=B, T=T, F=F, N=N, n_fixed=N0, iters=a.iters,
                        median_ms=float(np.median(ms)), repeats_ms=[float(v) for v in ms])
            if name == "adapt":
                line["workspace_MiB"] = ws.numel() / 2.0 ** 20
                line["max_abs_dW_vs_loop_last_row"] = float((got["adapt"][1][B - 1] - got["loop_W_last"]).abs().max())
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
