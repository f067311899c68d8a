"""Wall time of the sparse-NMF baseline's inference, both paths of ops.snmf_mask_forward in one session.

    python tools/snmf_bench.py [--iters 200] [--rows 32,4096,262144] [--out profiles/snmf_bench.jsonl]
                               [--root CHECKOUT] [--label NAME] [--beta 2|1]

At the shipped dictionary size (F = 257, N = 200) and the reference's 200 iterations (enhance.py:842), for
n = 32, 4096 and 262144 frame rows: median milliseconds of
  gemm     path = 1: pack kernel, drnmf_mu_forward's launches (three device-wide products per iteration), zero kernel
  tile     path = 2: one launch, a workgroup per 16 rows for all iterations
  f16      ops.snmf_f16_forward: the tile kernel's structure on fp16 matrix-core operands (where the measured
           package has it), with its largest mask difference from the tile path
  mu       ops.mu_forward with want_irm on the same input -- the entry the package had before, measured before and
           after the paths to show drift inside the session.
--beta 1 measures the KL cost instead: the GEMM path at beta = 1 and the KL tile kernel (ops.snmf_kl_forward, path
name 'kl', with its largest mask difference from the GEMM path), between the same two `mu` runs at beta = 1; every
line then carries "beta": 1.0.  _capi.SNMF_KL_AUTO_MAX_ROWS is read off such a session.
--root measures the package of ANOTHER checkout (built there) with this script -- the parent commit's, in front of
and behind this one's, is how a session shows that the machine did not drift between two builds; --label names the
run in the JSON lines.
Every configuration is warmed once and timed with device events; one JSON line per (rows, path) is appended to
--out.  Nothing is asserted about speed; the largest difference of the two paths' masks is reported with them."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F, N, SPARSITY = 257, 200, 1.0


def timed(fn, reps, prepare=None):
    """Milliseconds of `reps` runs of fn, each between device events; prepare() runs outside the timed window."""
    out = []
    for _ in range(reps):
        if prepare is not None:
            prepare()
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
    ap.add_argument("--rows", default="32,4096,262144")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snmf_bench.jsonl"))
    ap.add_argument("--root", default=ROOT, help="the checkout whose package is measured (default: this one)")
    ap.add_argument("--label", default=None, help="written into every JSON line as 'label'")
    ap.add_argument("--beta", type=float, default=2.0, choices=[2.0, 1.0], help="2: 'ed' (default), 1: 'kl'")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import __graft_entry__ as G
    G.build()
    if not torch.cuda.is_available():
        raise RuntimeError("snmf_bench needs a GPU: a time taken anywhere else says nothing")
    from drnmf_amd import ops
    dev = "cuda:0"
    rng = np.random.RandomState(0)
    W = (rng.rand(F, N) ** 2 + 0.02).astype(np.float32)
    nrm = np.sqrt((W.astype(np.float64) ** 2).sum(axis=0))
    Wd = torch.from_numpy(W).to(dev)
    Wn = torch.from_numpy((W / nrm).astype(np.float32)).to(dev)
    h_init = rng.rand(N).astype(np.float32)
    hn = torch.from_numpy((h_init * nrm).astype(np.float32)).to(dev)
    h0 = torch.from_numpy(h_init).to(dev)
    lines = []
    for n in [int(v) for v in a.rows.split(",")]:
        g = torch.Generator(device=dev).manual_seed(n)
        x = torch.rand((1, n, F), generator=g, device=dev) ** 2 + 1e-3
        ws = torch.empty(max(1, ops._capi.lib().drnmf_snmf_mask_workspace_bytes(1, n, F, N)), dtype=torch.uint8,
                         device=dev)
        out = {p: torch.empty_like(x) for p in ("gemm", "tile", "f16", "kl")}
        H = torch.empty((n, N), dtype=torch.float32, device=dev)
        fill = lambda: H.copy_(h0[None].expand(n, N))
        runs = [("mu_before", lambda: ops.mu_forward(x[0], Wd, H, SPARSITY, a.iters, beta=a.beta, want_irm=True), fill)]
        for p in ("gemm", "tile") if a.beta == 2.0 else ("gemm",):
            runs.append((p, (lambda p=p: ops.snmf_mask_forward(x, Wn, hn, SPARSITY, a.iters, beta=a.beta,
                                                               mask_value=-1.0, path=p, out=out[p], workspace=ws)),
                         None))
        if a.beta == 1.0:
            wk = torch.empty(ops._capi.lib().drnmf_snmf_kl_workspace_bytes(), dtype=torch.uint8, device=dev)
            runs.append(("kl", lambda: ops.snmf_kl_forward(x, Wn, hn, SPARSITY, a.iters, mask_value=-1.0,
                                                           out=out["kl"], workspace=wk), None))
        elif hasattr(ops, "snmf_f16_forward"):
            d16 = ops.snmf_f16_pack_dict(Wn)
            runs.append(("f16", lambda: ops.snmf_f16_forward(x, d16, Wn, hn, SPARSITY, a.iters, mask_value=-1.0,
                                                             out=out["f16"]), None))
        runs.append(("mu_after", runs[0][1], fill))
        for name, fn, prep in runs:
            timed(fn, 1, prep)                       # warm-up: code objects, workspaces
            ms = timed(fn, a.reps, prep)
            line = dict(tool="snmf_bench", path=name, rows=n, F=F, N=N, iters=a.iters, median_ms=float(np.median(ms)),
                        repeats_ms=[float(v) for v in ms])
            if a.label is not None:
                line["label"] = a.label
            if a.beta != 2.0:
                line["beta"] = a.beta
            if name in ("tile", "kl"):
                line["max_abs_diff_vs_gemm"] = float((out[name] - out["gemm"]).abs().max())
            if name == "f16":
                line["max_abs_diff_vs_tile"] = float((out["f16"] - out["tile"]).abs().max())
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
