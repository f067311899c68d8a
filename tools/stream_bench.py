"""Per-push wall time and throughput of model.stream against the host-framed alternative.

    python tools/stream_bench.py [--family lstm|snmf] [--seconds 4] [--out profiles/stream_bench.jsonl]

For 1 and 64 streams of 16 kHz audio and pushes of 10 ms / 100 ms / 1 s: the same audio through
  stream   model.stream(...).push per chunk (carry on the device), and
  host     the framing a user had to write before: the carry of N - hop input samples and N - hop partial sums
           kept in numpy, ops.stft of the carried window per chunk, predict_on_batch, ops.istft_masked, the
           overlap tail added on the host.
Every configuration runs 5 times, synchronised; the JSON line holds the median and all repeats.  Nothing is
asserted about speed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FS, N, HOP, F = 16000, 512, 128, 257


def build_model(family, device):
    from drnmf_amd import layers
    from oracle import drnmf_oracle as O
    if family == "snmf":
        r = 16
        P = O.synth_problem(2, 4, F, r, seed=3)
        params = dict(input_dim=F, hidden_dim=2 * r, output_dim=F, mask_value=-1., maxseq=200, K_layers=3,
                      W=P["W"], alph=2 * r / 4.0, lam1=0.3, params_untied=["log_D", "log_alph"],
                      params_trainable=["log_D", "log_alph"])
        model = layers.build_unfolded_snmf(params, device=device)
        model.cell.stateful = True
        return model
    torch.manual_seed(0)
    np.random.seed(0)
    return layers.build_lstm(dict(mask_value=-1., maxseq=200, input_dim=F, output_dim=F, K_layers=2, hidden_dim=48,
                                  stateful=True), device=device)


def run_stream(model, audio, chunk):
    st = model.stream(audio.shape[0], N=N, hop=HOP, dtype="float32", crop=True)
    times = []
    for p in range(0, audio.shape[1], chunk):
        t0 = time.perf_counter()
        st.push(list(audio[:, p:p + chunk]))        # (push ends with a synchronised copy down)
        times.append(time.perf_counter() - t0)
    st.close()
    return times


def run_host(model, audio, chunk, device):
    """Host-side framing: `buf` holds the zero-prefixed samples no emitted frame has left behind; the frames that
    are complete go through ops.stft as a signal of their own (whose first N / hop frames reach into its own
    leading zeros and are dropped), the model, and ops.istft_masked between zero frames (so that its trimming
    keeps every sample); the N - hop samples later frames still add to wait in numpy."""
    from drnmf_amd import ops
    B, k0 = audio.shape[0], N // HOP
    model.reset_states(batch_size=B)
    buf = np.zeros((B, N), np.float32)              # the N zeros in front of the stream
    tail = np.zeros((B, N - HOP), np.float32)
    times = []
    for p in range(0, audio.shape[1], chunk):
        t0 = time.perf_counter()
        buf = np.concatenate([buf, audio[:, p:p + chunk]], axis=1)
        n_new = (buf.shape[1] - N) // HOP + 1 if buf.shape[1] >= N else 0
        if n_new > 0:
            width = (n_new - 1) * HOP + N
            span = torch.from_numpy(np.ascontiguousarray(buf[:, :width])).to(device)
            re, im, mag = ops.stft(span, N=N, hop=HOP, want_mag=True)
            sl = slice(k0, k0 + n_new)
            mask = torch.from_numpy(model.predict_on_batch(mag[:, sl].cpu().numpy())).to(device)
            rp = torch.zeros((B, n_new + 2 * k0 + 1, F), dtype=torch.float32, device=device)
            ip, mp = torch.zeros_like(rp), torch.zeros_like(rp)
            rp[:, sl], ip[:, sl], mp[:, sl] = re[:, sl], im[:, sl], mask
            y = ops.istft_masked(rp, ip, mp, width, N, HOP).cpu().numpy()
            y[:, :N - HOP] += tail
            tail = y[:, n_new * HOP:].copy()        # y[:, :n_new * HOP] is final
            buf = buf[:, n_new * HOP:]
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", default="lstm", choices=["lstm", "snmf"])
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    device = "cuda:0"
    model = build_model(a.family, device)
    rng = np.random.default_rng(0)
    lines = []
    for B in (1, 64):
        audio = (0.1 * rng.standard_normal((B, int(a.seconds * FS)))).astype(np.float32)
        for ms in (10, 100, 1000):
            chunk = FS * ms // 1000
            for name, fn in (("stream", lambda: run_stream(model, audio, chunk)),
                             ("host", lambda: run_host(model, audio, chunk, device))):
                fn()                                # warm-up: graph captures, workspaces, pinned buffers
                reps = [float(np.median(fn())) for _ in range(5)]
                med = float(np.median(reps))
                line = dict(tool="stream_bench", family=a.family, path=name, streams=B, push_ms=ms,
                            push_wall_ms=1e3 * med, samples_per_s=B * chunk / med,
                            repeats_ms=[1e3 * r for r in reps])
                print(json.dumps(line), flush=True)
                lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
