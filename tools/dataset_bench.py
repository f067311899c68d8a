"""ops.wavs_to_tensors against the path composed of the per-file entry points, and the paired kernel against two
ragged launches: one JSON line, appended to profiles/dataset_bench.jsonl.

    python tools/dataset_bench.py [--utts 1980] [--reps 5] [--skip-e2e] [--skip-kernel] [--target mag|psa|tpsa]

The utterances are those of tools/enhance_bench.py: lengths drawn (seed 0) uniformly from 2 to 12 s at 16 kHz, int16
noise-like samples, the clean side a second draw of the same lengths; N = 512, hop = 128; maxlen None and 500.
Fields per maxlen:
  device_s / composed_s   median of --reps host-clock times of the whole call, each ending synchronised with the
                          tensors on the device, the two paths alternating in one process after one warm-up of
                          each; *_all lists every repeat.  composed = ops.stft per file (both sides) with the
                          magnitude brought to the host, data.reshape_and_pad_stacks, upload of x, y and the mask
  pcie_bytes              bytes over the link, computed from shapes: device = int16 samples of both sides up (+ 8
                          bytes of length per signal and side, 8 per sequence); composed = int16 up, float32
                          magnitudes of both sides down, padded x, y and mask up
  max_abs_diff            of x, y and w between the two paths (0: bitwise equal)
--target psa / tpsa (include/drnmf_target.h): the composed path has no such target and is not run; device_s is timed
alternating with target='mag' in the same process (mag_s, ratio = device_s / mag_s), x_w_equal_mag: x and w bitwise
those of 'mag'.
Paired kernel alone (device events, median of --reps after a warm-up), 250 pairs of 2000 frames, int16:
  pair_chunks_us, and ragged_x2_us = two drnmf_stft_ragged launches writing the same rows (which also write re and
  im: ragged_x2_bytes counts them), each with its bytes in + out over time as a share of the 8 TB/s HBM rate;
  pair_psa_us / pair_tpsa_us = drnmf_stft_pair_chunks_target on the same buffers (the same bytes), in the same run.
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

HBM_BYTES_PER_S = 8.0e12
N_FFT, HOP, F = 512, 128, 257
DEV = "cuda:0"


def composed(ops, data, noisy, clean, maxlen):
    """load_data out of the per-file entry points (what a caller had to write before wavs_to_tensors)."""
    xs, ys, fidx, t = [], [], [], 0
    for xw, yw in zip(noisy, clean):
        my = ops.stft(torch.from_numpy(yw).to(DEV), N=N_FFT, hop=HOP, want_mag=True)[2][0].cpu().numpy()
        mx = ops.stft(torch.from_numpy(xw).to(DEV), N=N_FFT, hop=HOP, want_mag=True)[2][0].cpu().numpy()
        xs.append(mx[:my.shape[0]].T)
        ys.append(my.T)
        fidx.append((t, t + my.shape[0]))
        t += my.shape[0]
    x, y, m = data.reshape_and_pad_stacks(np.concatenate(xs, axis=1), np.concatenate(ys, axis=1),
                                          np.asarray(fidx), pad_value=-1.0, maxlen=maxlen)
    return tuple(torch.from_numpy(a).to(DEV) for a in (x, y, np.ascontiguousarray(m[:, :, 0])))


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    del out
    return time.perf_counter() - t


def kernel_case(ops, n_sig, frames, reps):
    nsampl = (frames - N_FFT // HOP - 1) * HOP
    assert ops.stft_frames(nsampl, N_FFT, HOP) == frames
    g = torch.Generator(device=DEV)
    g.manual_seed(2)
    px = torch.randint(-20000, 20000, (n_sig, nsampl), generator=g, device=DEV, dtype=torch.int16)
    py = torch.randint(-20000, 20000, (n_sig, nsampl), generator=g, device=DEV, dtype=torch.int16)
    ld = torch.full((n_sig,), nsampl, dtype=torch.int64, device=DEV)
    idx = torch.arange(n_sig, dtype=torch.int32, device=DEV)
    table = torch.stack([idx, torch.zeros_like(idx)], dim=1).contiguous()
    shape = (n_sig, frames, F)
    x, y = (torch.empty(shape, dtype=torch.float32, device=DEV) for _ in range(2))
    w = torch.empty(shape[:2], dtype=torch.float32, device=DEV)
    x2, y2, re, im = (torch.empty(shape, dtype=torch.float32, device=DEV) for _ in range(4))

    def events(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts)), [round(t, 1) for t in ts]

    def two_ragged():
        ops.stft_ragged_enqueue(px, ld, idx, frames, N_FFT, HOP, -1.0, x2, re, im)
        ops.stft_ragged_enqueue(py, ld, idx, frames, N_FFT, HOP, -1.0, y2, re, im)

    pair, pair_all = events(lambda: ops.stft_pair_chunks_enqueue(px, py, ld, ld, table, frames, N_FFT, HOP, "mag",
                                                                 -1.0, x, y, w))
    rag, rag_all = events(two_ragged)
    same = bool(torch.equal(x, x2) and torch.equal(y, y2))
    targets = {}
    for target in ("psa", "tpsa"):
        t, t_all = events(lambda: ops.stft_pair_target_enqueue(px, py, ld, ld, table, frames, N_FFT, HOP, "mag", target,
                                                               -1.0, x, y, w))
        targets.update({"pair_%s_us" % target: round(t, 1), "pair_%s_us_all" % target: t_all,
                        "pair_%s_over_mag" % target: round(t / pair, 3)})
    pcm = 2 * n_sig * nsampl * 2
    pair_bytes = pcm + 2 * n_sig * frames * F * 4 + n_sig * frames * 4
    rag_bytes = pcm + 6 * n_sig * frames * F * 4
    return dict(n_sig=n_sig, frames=frames, N=N_FFT, hop=HOP, pair_chunks_us=round(pair, 1),
                pair_chunks_us_all=pair_all, ragged_x2_us=round(rag, 1), ragged_x2_us_all=rag_all,
                pair_bytes=pair_bytes, ragged_x2_bytes=rag_bytes,
                pair_hbm_share=round(pair_bytes / (pair * 1e-6) / HBM_BYTES_PER_S, 4),
                ragged_x2_hbm_share=round(rag_bytes / (rag * 1e-6) / HBM_BYTES_PER_S, 4), bitwise_equal=same,
                **targets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1980)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--target", choices=("mag", "psa", "tpsa"), default="mag")
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import data, ops
    if not torch.cuda.is_available():
        raise SystemExit("dataset_bench needs a GPU")
    fs, n = 16000, a.utts
    rng = np.random.default_rng(0)
    lengths = rng.integers(2 * fs, 12 * fs + 1, size=n).astype(np.int64)
    noisy = [rng.integers(-3000, 3000, size=int(l)).astype(np.int16) for l in lengths]
    clean = [rng.integers(-3000, 3000, size=int(l)).astype(np.int16) for l in lengths]
    res = dict(tool="dataset_bench", utts=n, fs=fs, lengths="uniform 2-12 s (seed 0)", N=N_FFT, hop=HOP,
               reps=a.reps, total_s=float(lengths.sum()) / fs, device=torch.cuda.get_device_name(0), target=a.target)
    if not a.skip_e2e:
        nf = np.array([ops.stft_frames(int(l), N_FFT, HOP) for l in lengths], dtype=np.int64)
        for maxlen in (None, 500):
            table, T = data.sequence_table_from_lengths(nf, maxlen)
            n_seq = table.shape[0]
            padded = n_seq * T * (2 * F + 1) * 4
            pcie = dict(device=int(4 * lengths.sum() + 16 * n + 8 * n_seq),
                        composed=int(4 * lengths.sum() + 2 * int(nf.sum()) * F * 4 + padded))
            dev_fn = lambda: ops.wavs_to_tensors(noisy, clean, N=N_FFT, hop=HOP, maxlen=maxlen, device=DEV,
                                                 target=a.target)
            if a.target != "mag":
                mag_fn = lambda: ops.wavs_to_tensors(noisy, clean, N=N_FFT, hop=HOP, maxlen=maxlen, device=DEV)
                got, want = dev_fn(), mag_fn()                           # warm-up of both
                same = bool(torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]))
                del got, want
                td, tm = [], []
                for _ in range(a.reps):
                    td.append(timed(dev_fn))
                    tm.append(timed(mag_fn))
                md, mm = float(np.median(td)), float(np.median(tm))
                res["maxlen_%s" % maxlen] = dict(
                    n_seq=int(n_seq), T=int(T), tensor_bytes=int(padded), device_s=round(md, 4), mag_s=round(mm, 4),
                    device_s_all=[round(t, 4) for t in td], mag_s_all=[round(t, 4) for t in tm],
                    ratio=round(md / mm, 3), pcie_bytes=pcie["device"], x_w_equal_mag=same)
                torch.cuda.empty_cache()
                continue
            cmp_fn = lambda: composed(ops, data, noisy, clean, maxlen)
            got, want = dev_fn(), cmp_fn()                               # warm-up of both paths
            diff = max(float((g - w).abs().max()) for g, w in zip(got, want))
            del got, want
            td, tc = [], []
            for _ in range(a.reps):
                td.append(timed(dev_fn))
                tc.append(timed(cmp_fn))
            md, mc = float(np.median(td)), float(np.median(tc))
            res["maxlen_%s" % maxlen] = dict(
                n_seq=int(n_seq), T=int(T), tensor_bytes=int(padded), device_s=round(md, 4), composed_s=round(mc, 4),
                device_s_all=[round(t, 4) for t in td], composed_s_all=[round(t, 4) for t in tc],
                speedup=round(mc / md, 2), pcie_bytes=pcie, max_abs_diff=diff)
            torch.cuda.empty_cache()
    if not a.skip_kernel:
        res["pair_kernel"] = kernel_case(ops, 250, 2000, a.reps)
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "dataset_bench.jsonl"), "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
