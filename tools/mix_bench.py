"""A fresh draw of training mixtures on the device (ops.MixBank.tensors) against the route a user had before it:
numpy mixing on the host, then ops.wavs_to_tensors on the pairs.  One JSON line, appended to
profiles/mix_bench.jsonl.

    python tools/mix_bench.py [--utts 512] [--noises 32] [--reps 15] [--mix-only K]

Workload: --utts utterances of 2 to 6 s at 16 kHz (lengths drawn with seed 0), --noises recordings of 60 s, int16
noise-like samples on both sides, SNRs uniform in [-6, 9] dB, N = 512, hop = 128, maxlen = 500.  After one warm-up of
each route the routes alternate --reps times in one process; every timed call ends in a synchronise and a new epoch's
draw is made for every repeat (outside the timed part; draw_s is its median).
  bank_s          (a) bank.tensors(draw, out=(x, y, w)): three index tables up, the mix, the pair kernels
  host_mix_s      (b1) the same mixtures in numpy float32 on the host: energies in float64, one gain per utterance
  tensors_i16_s   (b2) ops.wavs_to_tensors on those mixtures rounded to int16, with the int16 clean side: the
                  cheapest upload the old route has
  tensors_f32_s   (b2') the same on the float32 mixtures and a float32 clean side: what keeps the mixtures' precision
  required        bank_s <= 1.10 * tensors_i16_s (the smaller of the two): the same STFT launches, about three
                  passes over samples in device memory more, two pinned uploads fewer
  mix_us          device events around bank.mix alone (the three kinds of launch), median of --reps
  mix_bytes       algorithmic bytes of the two sample passes: segment energy = 2 per valid sample (int16 noise);
                  mix = 4 (speech) + 2 (noise) per valid sample + 4 per element of the padded output
  x_equal         x of (a) is bitwise that of wavs_to_tensors on bank.wavs(draw) and the float32 clean side
--mix-only K: K calls of bank.mix after a warm-up and nothing else (the body of a kernel-trace run).
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

N_FFT, HOP, MAXLEN, FS = 512, 128, 500, 16000
DEV = "cuda:0"


def host_mix(clean, noise, draw):
    """What a user wrote before: float32 mixtures, one utterance at a time."""
    out = []
    for s16, j, o, snr in zip(clean, *draw):
        s = s16.astype(np.float32) / np.float32(32768.0)
        z = noise[j]
        seg = np.take(z, np.arange(o, o + len(s)), mode='wrap').astype(np.float32) / np.float32(32768.0)
        es, en = np.sum(s.astype(np.float64) ** 2), np.sum(seg.astype(np.float64) ** 2)
        g = np.float32(np.sqrt(es / en) * 10.0 ** (-float(snr) / 20.0))
        out.append(s + g * seg)
    return out


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    del out
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=512)
    ap.add_argument("--noises", type=int, default=32)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--mix-only", type=int, default=0)
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench needs a GPU")
    rng = np.random.default_rng(0)
    lengths = rng.integers(2 * FS, 6 * FS + 1, size=a.utts).astype(np.int64)
    clean = [rng.integers(-3000, 3000, size=int(l)).astype(np.int16) for l in lengths]
    noise = [rng.integers(-3000, 3000, size=60 * FS).astype(np.int16) for _ in range(a.noises)]
    bank = ops.MixBank(clean, noise, device=DEV)
    draw = lambda ep: bank.draw(seed=1, epoch=ep)
    if a.mix_only:
        bank.mix(draw(0))
        torch.cuda.synchronize()
        for ep in range(a.mix_only):
            bank.mix(draw(1 + ep))
        torch.cuda.synchronize()
        return
    kw = dict(N=N_FFT, hop=HOP, maxlen=MAXLEN)
    clean32 = [v.astype(np.float32) / np.float32(32768.0) for v in clean]
    to_i16 = lambda ws: [np.clip(np.round(w * 32768.0), -32768, 32767).astype(np.int16) for w in ws]
    out = bank.tensors(draw(0), **kw)                                            # warm-up of every route
    want = ops.wavs_to_tensors(bank.wavs(draw(0)), clean32, device=DEV, **kw)
    x_equal = bool(all(torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(out, want)))
    mixed = host_mix(clean, noise, draw(0))
    host_diff = max(float(np.max(np.abs(m - w))) for m, w in zip(mixed, bank.wavs(draw(0))))
    del want
    ops.wavs_to_tensors(to_i16(mixed), clean, device=DEV, **kw)
    ops.wavs_to_tensors(mixed, clean32, device=DEV, **kw)
    t = dict(bank=[], host_mix=[], i16=[], f32=[], draw=[])
    for rep in range(a.reps):
        t0 = time.perf_counter()
        d = draw(1 + rep)
        t["draw"].append(time.perf_counter() - t0)
        t["bank"].append(timed(lambda: bank.tensors(d, out=out, **kw)))
        t0 = time.perf_counter()
        mixed = host_mix(clean, noise, d)
        t["host_mix"].append(time.perf_counter() - t0)
        mixed16 = to_i16(mixed)
        t["i16"].append(timed(lambda: ops.wavs_to_tensors(mixed16, clean, device=DEV, **kw)))
        t["f32"].append(timed(lambda: ops.wavs_to_tensors(mixed, clean32, device=DEV, **kw)))
    ev = []
    for rep in range(a.reps):
        d = draw(100 + rep)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        bank.mix(d)
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1) * 1e3)
    med = {k: float(np.median(v)) for k, v in t.items()}
    valid, padded = int(lengths.sum()), int(a.utts * lengths.max())
    res = dict(tool="mix_bench", utts=a.utts, noises=a.noises, fs=FS, lengths="uniform 2-6 s (seed 0)", N=N_FFT,
               hop=HOP, maxlen=MAXLEN, reps=a.reps, total_s=valid / FS, device=torch.cuda.get_device_name(0),
               n_seq=int(out[0].shape[0]), T=int(out[0].shape[1]),
               bank_s=round(med["bank"], 5), host_mix_s=round(med["host_mix"], 4), draw_s=round(med["draw"], 6),
               tensors_i16_s=round(med["i16"], 5), tensors_f32_s=round(med["f32"], 5),
               bank_s_all=[round(v, 5) for v in t["bank"]], tensors_i16_s_all=[round(v, 5) for v in t["i16"]],
               tensors_f32_s_all=[round(v, 5) for v in t["f32"]],
               ratio_i16=round(med["bank"] / med["i16"], 3), ratio_f32=round(med["bank"] / med["f32"], 3),
               required="bank_s <= 1.10 * tensors_i16_s", met=bool(med["bank"] <= 1.10 * med["i16"]),
               mix_us=round(float(np.median(ev)), 1), mix_us_all=[round(v, 1) for v in ev],
               mix_bytes=dict(segment_energy=2 * valid, mix=6 * valid + 4 * padded), x_equal=x_equal,
               host_mix_max_abs_diff=host_diff)
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mix_bench.jsonl"), "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
