"""Timing of the HuBERT-Soft units encoder (ddsp.hubert.HubertSoft.units -> ddsp_hubert_soft_units) at the GUI window (4.5 s),
10 s and 30 s of 16 kHz audio, in both product modes, next to a PyTorch-eager fp32 restatement of the same network on the
same weights (tests/hubert_cases.eager_units) - what a user of the reference pays on the same GPU.

    python tools/hubert_time.py [--form soft|cvec|cvec768] [--iters N] [--warmup W] [--lengths 72000,160000,480000] [--out file.json]

--form cvec / cvec768 times the base form instead (ddsp.hubert.HubertBase.units -> ddsp_hubert_base_units: no padding, 9 of
the 12 transformer layers, with / without the final projection) on a deterministic fill of its own keys; there is no eager
baseline and no TFLOP/s for it (the count below is the 12-layer network's).

Every call is bracketed by device events after W warm-up calls; mean and p99 of N calls.  TFLOP/s from the issue's count:
13.9 GFLOP per second of audio for the linear part plus 36 864 L^2 for the attention (L encoder frames)."""
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
import hubert_cases as HC  # noqa: E402
from ddsp.hubert import HubertBase, HubertSoft, n_frames  # noqa: E402


def flops(T):
    L = n_frames(T)
    return 13.9e9 * T / 16000 + 36864.0 * L * L


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
    ap.add_argument("--lengths", default="72000,160000,480000")
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--form", default="soft", choices=["soft", "cvec", "cvec768"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    soft = a.form == "soft"
    m = HubertSoft() if soft else HubertBase()
    run = m.units if soft else (lambda x: m.units(x, layer=9, project=a.form == "cvec"))
    frames = n_frames if soft else HubertBase.frames
    m.load_state_dict(HC.fill({k: tuple(v.shape) for k, v in m.state_dict().items()}))
    m = m.to(dev).eval()
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    ctx = hipddsp.context_for(dev)
    rows = []
    for T in [int(t) for t in a.lengths.split(",")]:
        x = (0.1 * torch.randn(1, 1, T, generator=torch.Generator().manual_seed(T))).to(dev)
        f = flops(T) if soft else None
        for name, math in (("split_bf16", hipddsp.MATH_SPLIT_BF16), ("fp32", hipddsp.MATH_FP32)):
            ctx.set_math(math)
            mean, p99 = timed(lambda: run(x), a.iters, a.warmup)
            rows.append({"impl": f"hip_{name}", "form": a.form, "T": T, "seconds": T / 16000, "frames": frames(T), "mean_ms": mean,
                         "p99_ms": p99, "tflops": f / mean * 1e-9 if soft else None})
            print(json.dumps(rows[-1]), flush=True)
        ctx.set_math(hipddsp.MATH_SPLIT_BF16)
        if soft and not a.no_eager:
            with torch.inference_mode():
                mean, p99 = timed(lambda: HC.eager_units(sd, x[:, 0]), a.iters, a.warmup)
            rows.append({"impl": "torch_eager_fp32", "T": T, "seconds": T / 16000, "frames": n_frames(T), "mean_ms": mean,
                         "p99_ms": p99, "tflops": f / mean * 1e-9})
            print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
