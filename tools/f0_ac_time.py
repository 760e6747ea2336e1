"""Timing of the autocorrelation f0 extractor (ddsp.vocoder.F0_Extractor('ac').extract on a device tensor) next to the CREPE
extractor ('full' network, deterministic fill of tests/crepe_cases.py) in the same session on the same GPU, at the GUI's
analysed span (a 4.5 s window at 44.1 kHz with silence_front 2.97 s: 1.54 s) and at a 0.2 s-block window (config5 of
tests/test_gpu_stream_chain.py: a 1.0 s window, nothing cropped), bounds 50..1100 Hz as `realtime.StreamRenderer` passes them.

    python tools/f0_ac_time.py [--iters N] [--warmup W] [--cases gui,block] [--out file.json]

Every call is bracketed by device events after W warm-up calls; mean and p99 of N calls.  `extract` only: the real-time
chain and the bank with `f0_extractor="ac"` are not timed here."""
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
from crepe_time import timed  # noqa: E402

SR, HOP, F0_MIN, F0_MAX = 44100, 512, 50, 1100
CASES = {"gui": (4.5, 2.97), "block": (1.0, 0.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="gui,block")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = Crepe("full")
    model.load_state_dict(CC.fill("full"))
    ex = {"ac": F0_Extractor("ac", SR, HOP, F0_MIN, F0_MAX, device=dev),
          "crepe": F0_Extractor("crepe", SR, HOP, F0_MIN, F0_MAX, crepe_ckpt=model.to(dev).eval(), device=dev)}
    rows = []
    for name in a.cases.split(","):
        seconds, sf = CASES[name]
        T = int(SR * seconds)
        t = torch.arange(T, dtype=torch.float64) / SR
        x = (0.3 * torch.sin(2 * np.pi * 160 * t * (1 + 0.1 * t)) + 0.01 * torch.randn(T, generator=torch.Generator().manual_seed(T),
                                                                                     dtype=torch.float64)).float().to(dev)
        n_frames, start_frame, crop = CC.extract_bookkeeping(T, SR, HOP, sf)
        for impl, e in ex.items():
            mean, p99 = timed(lambda: e.extract(x, uv_interp=True, silence_front=sf, dither=False), a.iters, a.warmup)
            row = {"case": name, "impl": impl, "seconds_analysed": (T - crop) / SR, "frames": n_frames, "mean_ms": mean, "p99_ms": p99}
            if impl == "ac":
                row["analysis_frames"] = hipddsp.f0_ac_frames(T - crop, SR, HOP, F0_MIN)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
