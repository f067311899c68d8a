"""LSTM baseline timings: one JSON line per shipped configuration (data_setup_downsample*/configs/
params_lstm_*.yaml: K_layers / hidden_dim = 5/250, 2/54, 5/70, 2/244) at F = 513, T = 500.

    python tools/lstm_bench.py [--reps N] [--config I]

  hip_forward_ms_b250       LSTMModel.forward at B = 250 (Masking -> K LSTM -> Dense -> sigmoid), device tensors
                            in and out, hard_sigmoid gates (the Keras default)
  hip_predict_slab_ms_b250  LSTMModel.predict(x, batch_size=250) of 250 full-length utterances: ONE slab of
                            enhance.py's predict loop, host numpy in and out (staging and copies included)
  hip_forward_ms_b32        LSTMModel.forward at B = 32 (the training batch size)
  torch_lstm_ms_b{250,32}   torch.nn.LSTM(F, H, K, batch_first) forward at the same shapes -- a YARDSTICK, a
                            different model: sigmoid gates, no masking, full-length sequences, no head
  train_step_ms_b32         LSTMModel.train_on_batch at B = 32 with the reference's Adam(lr=1e-4, clipnorm=1.0):
                            training forward, loss head, BPTT, weight gradients and the fused Adam
  torch_train_step_ms_b32   torch.nn.LSTM + Linear + sigmoid, mse loss, autograd and torch.optim.Adam at the same
                            shapes -- the training YARDSTICK (sigmoid gates, no masking, no gradient clipping)
Medians of --reps timed calls (CUDA events; wall clock for predict, which synchronises) after two warm-up calls.
JSON lines go to stdout, nothing else does.
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

CONFIGS = [(5, 250), (2, 54), (5, 70), (2, 244)]
F, T = 513, 500


def _time(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--config", type=int, default=None, help="index into %s" % (CONFIGS,))
    args = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import layers
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    cfgs = CONFIGS if args.config is None else [CONFIGS[args.config]]
    for K, H in cfgs:
        m = layers.build_lstm(dict(mask_value=-1., maxseq=T, input_dim=F, output_dim=F, K_layers=K,
                                   hidden_dim=H), device=dev)
        net = torch.nn.LSTM(F, H, num_layers=K, batch_first=True).to(dev)
        line = dict(K_layers=K, hidden_dim=H, F=F, T=T)
        for B in (250, 32):
            x = torch.from_numpy(rng.random((B, T, F), dtype=np.float32)).to(dev)
            hip = _time(lambda: m.forward(x), args.reps)
            with torch.no_grad():
                ref = _time(lambda: net(x), args.reps)
            line["hip_forward_ms_b%d" % B] = round(hip, 3)
            if B == 250:
                xh = x.cpu().numpy()
                for _ in range(2):
                    m.predict(xh, batch_size=250)
                ts = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    m.predict(xh, batch_size=250)
                    ts.append(1e3 * (time.perf_counter() - t0))
                line["hip_predict_slab_ms_b250"] = round(float(np.median(ts)), 3)
            line["torch_lstm_ms_b%d" % B] = round(ref, 3)
            line["hip_over_torch_b%d" % B] = round(hip / ref, 3)
            del x
        B = 32
        x = rng.random((B, T, F), dtype=np.float32)
        y = rng.random((B, T, F), dtype=np.float32)
        xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        wd = torch.ones((B, T), dtype=torch.float32, device=dev)
        m.compile(lr=1e-4, clipnorm=1.0)
        line["train_step_ms_b32"] = round(_time(lambda: m.train_on_batch(xd, yd, wd), args.reps), 3)
        lin = torch.nn.Linear(H, F).to(dev)
        opt = torch.optim.Adam(list(net.parameters()) + list(lin.parameters()), lr=1e-4)

        def torch_step():
            opt.zero_grad(set_to_none=True)
            out = torch.sigmoid(lin(net(xd)[0]))
            loss = ((xd * out - yd) ** 2).mean()
            loss.backward()
            opt.step()
        line["torch_train_step_ms_b32"] = round(_time(torch_step, args.reps), 3)
        line["train_hip_over_torch_b32"] = round(line["train_step_ms_b32"] / line["torch_train_step_ms_b32"], 3)
        del xd, yd, wd, lin, opt
        line["yardstick"] = "torch.nn.LSTM: sigmoid gates, unmasked full-length input, no head (a different model)"
        print(json.dumps(line), flush=True)
        m.free_predict_buffers()
        del m, net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
