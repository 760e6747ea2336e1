"""Per-block time of `realtime.StreamRenderer`'s chain on one GPU (the device half of gui.py's audio callback), mean and p99
over N blocks after warm-up, each block timed from its push to its (block,) output being ready on the device - what the
callback waits for before it copies the block out.

Two shapes: BASELINE config #5 (0.2 s block, buffer 4, 0.04 s cross-fade) and gui.py's Config defaults (1.5 s block, buffer 2,
0.03 s cross-fade), both with a 44.1 kHz CombSub model (seeded random weights), the forward replayed from a HIP graph.
Legs per shape: the model only (44.1 kHz device); a 48 kHz device (fractional-hop volume + 44.1 -> 48 kHz resampling before
the splice); the enhancer at the shipped NSF-HiFiGAN geometry (seeded random weights) with key 0 and with 'auto' (a track
peaking at 1000 Hz: key 5, so the generator runs at a shifted rate between two resamplings); a speaker mix in the graph.

    python tools/rt_chain.py [--blocks N] [--warmup W] [--out result.json]"""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ddsp-svc-official_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import glue_cases as GC
import realtime
import synthetic
from enhancer import Enhancer

SHIPPED = dict(GC.NSF_CONFIG, upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4],
               upsample_initial_channel=512, num_mels=128, hop_size=512, n_fft=2048, win_size=2048)
SHAPES = {"config5": (0.2, 0.04, 4), "gui_defaults": (1.5, 0.03, 2)}
LEGS = {  # name: (device rate, enhancer key (None = off), speaker mix)
    "model": (44100, None, None),
    "device_48k": (48000, None, None),
    "enhancer_key0": (44100, 0, None),
    "enhancer_auto": (44100, "auto", None),
    "mix_graph": (44100, None, {1: 0.3, 3: 0.7}),
}


def shipped_enhancer(dev, tmp):
    with open(os.path.join(tmp, "config.json"), "w") as fh:
        json.dump(SHIPPED, fh)
    torch.save({"generator": GC.nsf_state_dict(SHIPPED, seed=91)}, os.path.join(tmp, "model"))
    with contextlib.redirect_stdout(sys.stderr):
        return Enhancer("nsf-hifigan", os.path.join(tmp, "model"), device=dev)


def time_leg(model, enh, dev, shape, leg, blocks, warmup):
    block_time, xfade_time, buffer_num = SHAPES[shape]
    sr, key, mix = LEGS[leg]
    r = realtime.StreamRenderer(model, sr, block_time, xfade_time, dev, buffer_num=buffer_num, threshold_db=-60.0, spk_id=1,
                                use_graph=True, spk_mix_dict=mix, enhancer=enh if key is not None else None,
                                enhancer_adaptive_key="auto" if key is None else key)
    feat = {k: v.to(dev) for k, v in synthetic.make_inputs(5, 1, r.frames, with_noise=False).items()}
    # a voiced track peaking at 1000 Hz after the enhancer's front cut ('auto' -> key 5)
    f0 = (250.0 + 750.0 * torch.sin(torch.arange(r.frames) / 7.0) ** 2).reshape(1, -1, 1).to(dev)
    rng = np.random.Generator(np.random.PCG64(3))
    pcm = [torch.from_numpy((0.2 * rng.standard_normal(r.block)).astype(np.float32)).to(dev) for _ in range(8)]
    times = []
    for i in range(warmup + blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.push_block(pcm[i % len(pcm)], units=feat["units"], f0=f0)
        torch.cuda.synchronize()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    t = np.array(times)
    return {"shape": shape, "leg": leg, "device_sr": sr, "block_ms": block_time * 1e3, "frames": r.frames,
            "key": r.last_key, "mean_ms": float(t.mean()), "p99_ms": float(np.percentile(t, 99)), "blocks": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rt_chain needs a HIP device")
    dev = torch.device("cuda:0")
    with contextlib.redirect_stdout(sys.stderr):
        model, _ = synthetic.build_model("CombSub", seed=1, device=dev)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        enh = shipped_enhancer(dev, tmp)
        for shape in SHAPES:
            for leg in LEGS:
                row = time_leg(model, enh, dev, shape, leg, a.blocks, a.warmup)
                rows.append(row)
                print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
