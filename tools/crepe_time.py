"""Timing of the CREPE f0 extractor (ddsp.vocoder.F0_Extractor('crepe').extract on a device tensor) at the GUI's analysed span
(a 4.5 s window at 44.1 kHz with silence_front 2.97 s: 1.54 s, 308 CREPE frames), at 10 s and at 30 s, in both product modes,
split into the network (`Crepe.activations`), the decode (`ddsp_crepe_decode`) and the post-filter (`ddsp_f0_postfilter`),
next to a PyTorch-eager fp32 restatement of the same 'full' network on the same GPU and weights (tests/crepe_cases.network):
what torchcrepe.infer costs a user of the reference there (its Viterbi then runs on the host, which this tool does not time).

    python tools/crepe_time.py [--iters N] [--warmup W] [--cases gui,10s,30s] [--no-eager] [--out file.json]

Every call is bracketed by device events after W warm-up calls; mean and p99 of N calls.  TFLOP/s from the network's count
(2.82 GFLOP per frame for 'full')."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ddsp-svc-official_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import hipddsp  # noqa: E402
import crepe_cases as CC  # noqa: E402
from ddsp.crepe import Crepe  # noqa: E402
from ddsp.vocoder import F0_Extractor  # noqa: E402

SR, HOP = 44100, 512
# name -> (seconds of audio at 44.1 kHz, silence_front)
CASES = {"gui": (4.5, 2.97), "10s": (10.0, 0.0), "30s": (30.0, 0.0)}


def net_flops(frames):
    w = CC.WIDTHS["full"]
    c_in = (1,) + w[:-1]
    pos = [256 >> i for i in range(6)]
    f = sum(2.0 * pos[i] * w[i] * c_in[i] * CC.KERNELS[i] for i in range(6)) + 2.0 * 4 * w[5] * 360
    return f * frames


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.array(ms)
    return float(ms.mean()), float(np.percentile(ms, 99))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="gui,10s,30s")
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = CC.fill("full")
    model = Crepe("full")
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    ex = F0_Extractor("crepe", SR, HOP, 65, 800, crepe_ckpt=model, device=dev)
    ctx = hipddsp.context_for(dev)
    sd32 = {k: v.to(dev) for k, v in sd.items() if v.dtype.is_floating_point}
    rows = []
    for name in a.cases.split(","):
        seconds, sf = CASES[name]
        T = int(SR * seconds)
        t = torch.arange(T, dtype=torch.float64) / SR
        x = (0.3 * torch.sin(2 * np.pi * 160 * t * (1 + 0.1 * t)) + 0.01 * torch.randn(T, generator=torch.Generator().manual_seed(T),
                                                                                     dtype=torch.float64)).float().to(dev)
        n_frames, start_frame, crop = CC.extract_bookkeeping(T, SR, HOP, sf)
        x16 = ctx.resample(x[crop:].reshape(1, -1), SR, 16000, lowpass_filter_width=128)
        fr = hipddsp.crepe_frames(x16.shape[-1])
        base = {"case": name, "seconds_analysed": x16.shape[-1] / 16000, "crepe_frames": fr}
        for mname, math in (("split_bf16", hipddsp.MATH_SPLIT_BF16), ("fp32", hipddsp.MATH_FP32)):
            ctx.set_math(math)
            probs = model.activations(x16)
            f0, pd = ctx.crepe_decode(probs, 65, 800, segment=512)
            parts = {
                "extract": lambda: ex.extract(x, uv_interp=True, silence_front=sf, dither=False),
                "network": lambda: model.activations(x16),
                "decode": lambda: ctx.crepe_decode(probs, 65, 800, segment=512),
                "postfilter": lambda: ctx.f0_postfilter(f0, pd, SR, HOP, n_frames, start_frame, 0.05, True, 65),
            }
            for part, fn in parts.items():
                mean, p99 = timed(fn, a.iters, a.warmup)
                row = dict(base, impl=f"hip_{mname}", part=part, mean_ms=mean, p99_ms=p99)
                if part == "network":
                    row["tflops"] = net_flops(fr) / mean * 1e-9
                if part == "decode":
                    row["us_per_frame"] = mean * 1e3 / fr
                rows.append(row)
                print(json.dumps(row), flush=True)
        ctx.set_math(hipddsp.MATH_SPLIT_BF16)
        if not a.no_eager:
            with torch.inference_mode():
                def eager():   # in batches of 512 frames, as the reference's torchcrepe.predict(..., batch_size=512)
                    fx = CC.frames(x16)
                    return torch.cat([CC.network(sd32, fx[i:i + 512]) for i in range(0, fx.shape[0], 512)]).reshape(1, -1, 360)
                mean, p99 = timed(eager, a.iters, a.warmup)
            row = dict(base, impl="torch_eager_fp32", part="network", mean_ms=mean, p99_ms=p99,
                       tflops=net_flops(fr) / mean * 1e-9)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
