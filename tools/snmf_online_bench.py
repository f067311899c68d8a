"""Wall time of the online noise-adaptive sparse-NMF baseline, per push, against the audio a push covers.

    python tools/snmf_online_bench.py [--iters 200] [--batches 1,4,16] [--pushes 4,64] [--frames 500] [--reps 5]
                                      [--block 64] [--w-iter 1] [--out profiles/snmf_online_bench.jsonl]

At the shipped dictionary size (F = 257, N = 200, the 100 speech atoms fixed), block 64 and the reference's 200
iterations, for B = 1, 4 and 16 streams, device events, median of --reps:
  online   ops.snmf_online_forward in pushes of 4 and of 64 frames.  A repeat is one run of pushes over two blocks
           (128 frames) from a reset state; every push is timed on its own.  Reported: the mean push of a run (the
           block updates spread over the pushes that fill a block) and the slowest push of a run (the one that
           completes a block), each as the median over the repeats; and one call of --frames frames.
  fixed    ops.snmf_mask_forward on the frames of one push / of the one call: the baseline without adaptation
  adapt    ops.snmf_adapt_forward on the --frames frames: the batch mode, which cannot be pushed
`audio_ms` is what a push covers at hop 128, 16 kHz (8 ms per frame); `realtime` is audio_ms / the slowest push.
One JSON line per (B, path, frames per call) is appended to --out.  Nothing is asserted about speed."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F, N, N0, SPARSITY, FRAME_MS = 257, 200, 100, 0.1, 8.0


def timed_each(fns):
    """Milliseconds of every callable of the list, run back to back, by device events."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)]
    ev[0].record()
    for k, fn in enumerate(fns):
        fn()
        ev[k + 1].record()
    ev[-1].synchronize()
    return [ev[k].elapsed_time(ev[k + 1]) for k in range(len(fns))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--pushes", default="4,64")
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--block", type=int, default=64)
    ap.add_argument("--w-iter", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snmf_online_bench.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    if not torch.cuda.is_available():
        raise RuntimeError("snmf_online_bench needs a GPU: a time taken anywhere else says nothing")
    from drnmf_amd import ops
    dev = "cuda:0"
    rng = np.random.RandomState(0)
    W = rng.rand(F, N) + 0.05
    Wn = torch.from_numpy((W / np.sqrt((W * W).sum(0))).astype(np.float32)).to(dev)
    hn = torch.from_numpy(rng.rand(N).astype(np.float32)).to(dev)
    T, L = a.frames, a.block
    lines = []

    def emit(**kw):
        line = dict(tool="snmf_online_bench", F=F, N=N, n_fixed=N0, iters=a.iters, block=L, w_iter=a.w_iter, **kw)
        print(json.dumps(line), flush=True)
        lines.append(line)

    for B in [int(v) for v in a.batches.split(",")]:
        g = torch.Generator(device=dev).manual_seed(B)
        x = torch.rand((B, max(T, 2 * L), F), generator=g, device=dev) ** 2 + 1e-3
        state = ops.snmf_online_state(B, F, N, N0, L, Wn, dev)
        online = lambda xs, ws: ops.snmf_online_forward(xs, hn, SPARSITY, a.iters, N0, state, w_iter=a.w_iter,
                                                        mask_value=-1.0, workspace=ws)
        fixed = lambda xs: ops.snmf_mask_forward(xs, Wn, hn, SPARSITY, a.iters, mask_value=-1.0)
        for P in [int(v) for v in a.pushes.split(",")] + [T]:
            whole = P == T
            span = T if whole else 2 * L
            cuts = [x[:, at:at + P].contiguous() for at in range(0, span, P)]
            ws = ops.snmf_online_workspace(B, P, F, N, N0, L, dev)
            runs = []
            for rep in range(a.reps + 1):            # the first run warms up: code objects, attributes
                ops.snmf_online_reset(state, Wn)
                ms = timed_each([lambda c=c: online(c, ws) for c in cuts])
                if rep:
                    runs.append(ms)
            timed_each([lambda: fixed(cuts[0])])
            fx = [timed_each([lambda: fixed(cuts[0])])[0] for _ in range(a.reps)]
            mean_ms = float(np.median([np.mean(r) for r in runs]))
            worst_ms = float(np.median([np.max(r) for r in runs]))
            audio = P * FRAME_MS
            emit(path="online", B=B, frames_per_call=P, calls_per_run=len(cuts), mean_push_ms=mean_ms,
                 slowest_push_ms=worst_ms, audio_ms=audio, realtime=audio / worst_ms,
                 launches_per_call=2 + ((P + 2 * L - 2) // L) * (4 + 2 * a.w_iter),
                 runs_mean_ms=[float(np.mean(r)) for r in runs], runs_slowest_ms=[float(np.max(r)) for r in runs])
            emit(path="fixed", B=B, frames_per_call=P, median_ms=float(np.median(fx)), audio_ms=audio,
                 realtime=audio / float(np.median(fx)), repeats_ms=[float(v) for v in fx])
        xa = x[:, :T].contiguous()
        wsa = ops.snmf_adapt_workspace(B, T, F, N, N0, dev)
        adapt = lambda: ops.snmf_adapt_forward(xa, Wn, hn, SPARSITY, a.iters, N0, mask_value=-1.0, workspace=wsa)
        timed_each([adapt])
        ad = [timed_each([adapt])[0] for _ in range(a.reps)]
        emit(path="adapt", B=B, frames_per_call=T, median_ms=float(np.median(ad)), audio_ms=T * FRAME_MS,
             repeats_ms=[float(v) for v in ad])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
