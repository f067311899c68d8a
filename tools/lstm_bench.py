"""LSTM baseline timings: one JSON line per shipped configuration (data_setup_downsample*/configs/
params_lstm_*.yaml: K_layers / hidden_dim = 5/250, 2/54, 5/70, 2/244) at F = 513, T = 500.

    python tools/lstm_bench.py [--reps N] [--config I] [--operand-dtype float32|float16] [--forward-only]

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
  step_us_b{250,32}         (--forward-only) us per wavefront diagonal (one lstm_step_kernel launch, its place in the
                            replayed graph included): the slope of ops.lstm_forward (no head) between T = 250 and 500
  operand_dtype             'float32', or 'float16' (LSTM(operand_dtype='float16'): fp16 operands in the recurrent
                            products, inference only -- such a row has no training columns)
--forward-only leaves out the torch yardsticks, the predict slab and the training step, and adds step_us_b*; without
it the run and its columns are what they were, plus operand_dtype.
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


def _step_us(m, x, half, reps):
    """us per wavefront diagonal: the recurrence alone (ops.lstm_forward, no head) at T / 2 and T frames; the slope
    is one lstm_step_kernel launch"""
    from drnmf_amd import ops
    B, Tx, Fx = x.shape
    H, K, act = m.lstms[0].units, len(m.lstms), m.lstms[0].recurrent_activation
    ts = []
    for Tt in (Tx // 2, Tx):
        xs = x[:, :Tt].contiguous()
        desc = ops.make_lstm_desc(B, Tt, Fx, H, K, act, operand_f16=half)
        params = ops.lstm_prepare_params(desc, [l.kernel for l in m.lstms], [l.recurrent_kernel for l in m.lstms],
                                         [l.bias for l in m.lstms], m.dense.kernel, m.dense.bias)
        ws = ops.lstm_workspace(desc, x.device)
        ts.append(_time(lambda: ops.lstm_forward(xs, -1.0, params, desc, workspace=ws), reps))
    return 1e3 * (ts[1] - ts[0]) / (Tx - Tx // 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--config", type=int, default=None, help="index into %s" % (CONFIGS,))
    ap.add_argument("--operand-dtype", default="float32", choices=["float32", "float16"])
    ap.add_argument("--forward-only", action="store_true")
    args = ap.parse_args()
    half = args.operand_dtype == "float16"
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import layers
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    cfgs = CONFIGS if args.config is None else [CONFIGS[args.config]]
    for K, H in cfgs:
        m = layers.build_lstm(dict(mask_value=-1., maxseq=T, input_dim=F, output_dim=F, K_layers=K,
                                   hidden_dim=H, operand_dtype=args.operand_dtype), device=dev)
        line = dict(K_layers=K, hidden_dim=H, F=F, T=T, operand_dtype=args.operand_dtype)
        if not args.forward_only:
            net = torch.nn.LSTM(F, H, num_layers=K, batch_first=True).to(dev)
        for B in (250, 32):
            x = torch.from_numpy(rng.random((B, T, F), dtype=np.float32)).to(dev)
            hip = _time(lambda: m.forward(x), args.reps)
            line["hip_forward_ms_b%d" % B] = round(hip, 3)
            if args.forward_only:
                line["step_us_b%d" % B] = round(_step_us(m, x, half, args.reps), 2)
                del x
                continue
            with torch.no_grad():
                ref = _time(lambda: net(x), args.reps)
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
        if args.forward_only or half:        # (float16 is inference only: LSTMModel.compile refuses it)
            print(json.dumps(line), flush=True)
            m.free_predict_buffers()
            del m
            torch.cuda.empty_cache()
            continue
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
