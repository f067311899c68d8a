"""model.enhance against the loop composed of the per-utterance entry points, and the ragged inverse kernel
against drnmf_istft_masked: one JSON line, appended to profiles/enhance_bench.jsonl.

    python tools/enhance_bench.py [--utts 1980] [--reps 5] [--models snmf,lstm] [--skip-e2e] [--skip-kernel]

The utterances are those of tools/stoi_bench.py: lengths drawn (seed 0) uniformly from 2 to 12 s at 16 kHz, int16
noise-like samples; N = 512, hop = 128; models: build_unfolded_snmf r = 100 / K = 5 and build_lstm K = 5 / H = 250
with random weights (the arithmetic does not depend on them).  Fields per model:
  enhance_s / composed_s   median of --reps host-clock times of the whole call, each ending synchronised, the two
                           paths alternating in one process after one warm-up of each (every slab shape is then
                           compiled / captured); *_all lists every repeat
  utt_per_s                utterances / median
  pcie_bytes               bytes over the link, computed from shapes: enhance = int16 samples up + int16 samples
                           down (+ 20 bytes of lengths / lists per utterance); composed = int16 up, (n, T_max, F)
                           float32 magnitudes down, up again through predict, masks down and up again, int16 down
Inverse kernel alone (CUDA events, median of --reps after a warm-up), equal lengths:
  istft_ragged_us / istft_masked_us and bytes in + out over time as a share of the 8 TB/s HBM rate.
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


def build_model(layers, family):
    from oracle import drnmf_oracle as O
    if family == "snmf":
        r, K = 100, 5
        P = O.synth_problem(2, 4, F, r, seed=3)
        params = dict(input_dim=F, hidden_dim=2 * r, output_dim=F, mask_value=-1., maxseq=2000, K_layers=K,
                      W=P["W"], alph=2 * r / 4.0, lam1=0.3, params_untied=["log_D", "log_alph"],
                      params_trainable=["log_D", "log_alph"])
        return layers.build_unfolded_snmf(params, device="cuda:0")
    torch.manual_seed(0)
    np.random.seed(0)
    return layers.build_lstm(dict(mask_value=-1., maxseq=2000, input_dim=F, output_dim=F, K_layers=5,
                                  hidden_dim=250), device="cuda:0")


def composed(ops, model, wavs, batch_size):
    """enhance.py's loop out of the per-utterance entry points (what a caller had to write before enhance)."""
    dev = "cuda:0"
    specs, mags = [], []
    for w in wavs:
        re, im, mag = ops.stft(torch.from_numpy(w).to(dev), N=N_FFT, hop=HOP, want_mag=True)
        specs.append((re, im))
        mags.append(mag[0].cpu().numpy())
    nfs = [m.shape[0] for m in mags]
    x = np.full((len(wavs), max(nfs), F), -1.0, np.float32)
    for i, m in enumerate(mags):
        x[i, :nfs[i]] = m
    masks = model.predict(x, batch_size=batch_size, lengths=nfs)
    out = []
    for i, w in enumerate(wavs):
        n_out = -(-len(w) // HOP) * HOP
        m = torch.from_numpy(masks[i:i + 1, :nfs[i]]).to(dev)
        y = ops.istft_masked(specs[i][0], specs[i][1], m, n_out, N_FFT, HOP)
        out.append(ops.to_int16_wav(y[0]).cpu().numpy())
    return out


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def kernel_case(ops, n_sig, nsampl, N, hop, reps):
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    pcm = 0.3 * torch.randn((n_sig, nsampl), generator=g, device=dev)
    lens = [nsampl] * n_sig
    x, re, im, nf = ops.stft_ragged(pcm, lens, N=N, hop=hop)
    T = int(nf[0])
    mask = torch.rand(x.shape, generator=g, device=dev)
    n_out = int(ops.ragged_out_lengths(lens, N, hop)[0])
    y = torch.empty((n_sig, n_out), dtype=torch.float32, device=dev)
    ld = torch.tensor(lens, dtype=torch.int64, device=dev)
    idx = torch.arange(n_sig, dtype=torch.int32, device=dev)

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
        return float(np.median(ts))

    rag = events(lambda: ops.istft_ragged_enqueue(re, im, mask, ld, idx, N, hop, y, False))
    # (ops.istft_masked allocates its frames workspace inside the call; the caching allocator serves it from the
    # second call on, so the timed calls pay no hipMalloc)
    old = events(lambda: ops.istft_masked(re, im, mask, n_out, N, hop))
    err = float((ops.istft_masked(re, im, mask, n_out, N, hop) - y).abs().max() / y.abs().max())
    nbytes = 3 * n_sig * T * (N // 2 + 1) * 4 + n_sig * n_out * 4
    return dict(n_sig=n_sig, frames=T, N=N, hop=hop, istft_ragged_us=round(rag, 1), istft_masked_us=round(old, 1),
                bytes_in_out=nbytes, ragged_hbm_share=round(nbytes / (rag * 1e-6) / HBM_BYTES_PER_S, 4),
                masked_hbm_share=round(nbytes / (old * 1e-6) / HBM_BYTES_PER_S, 4),
                masked_workspace_bytes=n_sig * T * N * 4, rel_diff=err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1980)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=250)
    ap.add_argument("--models", default="snmf,lstm")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import layers, ops
    if not torch.cuda.is_available():
        raise SystemExit("enhance_bench needs a GPU")
    fs, n = 16000, a.utts
    rng = np.random.default_rng(0)
    lengths = rng.integers(2 * fs, 12 * fs + 1, size=n).astype(np.int64)
    wavs = [rng.integers(-3000, 3000, size=int(l)).astype(np.int16) for l in lengths]
    res = dict(tool="enhance_bench", utts=n, fs=fs, lengths="uniform 2-12 s (seed 0)", N=N_FFT, hop=HOP,
               batch_size=a.batch_size, reps=a.reps, total_s=float(lengths.sum()) / fs,
               device=torch.cuda.get_device_name(0))
    if not a.skip_e2e:
        nf = np.array([ops.stft_frames(int(l), N_FFT, HOP) for l in lengths])
        n_out = ops.ragged_out_lengths(lengths, N_FFT, HOP)
        spec = int(n) * int(nf.max()) * F * 4
        pcie = dict(enhance=int(2 * lengths.sum() + 2 * n_out.sum() + 20 * n),
                    composed=int(2 * lengths.sum() + 2 * n_out.sum() + int(nf.sum()) * F * 4 * 2 + 2 * spec))
        res["pcie_bytes"] = pcie
        for family in [m for m in a.models.split(",") if m]:
            model = build_model(layers, family)
            got = model.enhance(wavs, N=N_FFT, hop=HOP, batch_size=a.batch_size)       # warm-up of every slab shape
            want = composed(ops, model, wavs, a.batch_size)
            diff = max(int(np.max(np.abs(g.astype(int) - w.astype(int)))) for g, w in zip(got, want))
            te, tc = [], []
            for _ in range(a.reps):
                te.append(timed(lambda: model.enhance(wavs, N=N_FFT, hop=HOP, batch_size=a.batch_size)))
                tc.append(timed(lambda: composed(ops, model, wavs, a.batch_size)))
            me, mc = float(np.median(te)), float(np.median(tc))
            res[family] = dict(enhance_s=round(me, 4), composed_s=round(mc, 4),
                               enhance_s_all=[round(t, 4) for t in te], composed_s_all=[round(t, 4) for t in tc],
                               enhance_utt_per_s=round(n / me, 1), composed_utt_per_s=round(n / mc, 1),
                               max_int16_diff=diff)
            model.free_predict_buffers()
            del model
            torch.cuda.empty_cache()
    if not a.skip_kernel:
        res["inverse_kernel"] = [kernel_case(ops, 64, 160000, 1024, 256, a.reps),
                                 kernel_case(ops, 250, (2000 - 5) * 128, 512, 128, a.reps)]
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "enhance_bench.jsonl"), "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
