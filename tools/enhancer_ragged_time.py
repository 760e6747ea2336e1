"""Ragged NSF-HiFiGAN enhancer against the per-slice loop: 32 slices of 0.5 - 14 s (the slice set of tools/ragged_time.py and
tools/hubert_ragged_time.py, here as 44.1 kHz audio, 512 samples a frame), the shipped 8-8-2-2-2 geometry with seeded
weights, the context's default product arithmetic, adaptive_key = 0, one GPU session.

  (a) the per-slice loop, `enhance(slice_i)` 32 times, on the PARENT tree (--baseline-tree, a built checkout of the commit
      before this feature): what `render(enhancer_batch_samples=None)` did before;
  (b) the same loop on this tree: what the per-row masks cost a solo call;
  (c) ragged groups, one `enhance_batch` per group of `infer_offline.group_segments` over the sample lengths, at several
      `enhancer_batch_samples`.
(a) and (b) run in child processes of their own (each under its own time limit), alternating between the two trees, so that
a difference between the builds is measured minutes apart on one device; the spread of (a) against itself is the yardstick
for (b).  Device events around each whole set of calls, 3 warm-up rounds, 15 timed: median, min and max.  Writes
profiles/enhancer_ragged_time.json with the times, (a)/(c) and each grouping's padded-to-real sample ratio.

    python tools/enhancer_ragged_time.py [--baseline-tree /path/to/built/parent/checkout] [--out profiles/enhancer_ragged_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ap = argparse.ArgumentParser()
_ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enhancer_ragged_time.json"))
_ap.add_argument("--baseline-tree", default=None, help="a built checkout of the parent commit: leg (a)")
_ap.add_argument("--loop-only", action="store_true", help="(child process) time the per-slice loop of --tree, print JSON")
_ap.add_argument("--tree", default=ROOT)
_ap.add_argument("--rounds", type=int, default=2, help="child processes per tree, alternating")
ARGS = _ap.parse_args()
sys.path[:0] = [ARGS.tree, os.path.join(ARGS.tree, "ddsp-svc-official_amd"), os.path.join(ROOT, "tests")]

import glue_cases as GC  # noqa: E402

WARMUP, RUNS = 3, 15
BUDGETS = [700000, 1500000, 4000000]
HOP, SR = 512, 44100
CONFIG = dict(GC.NSF_CONFIG, upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4], upsample_initial_channel=512,
              num_mels=128, hop_size=512, n_fft=2048, win_size=2048)


def slice_frames():
    """The 32 slice lengths of tools/ragged_time.py, in frames of 512 samples at 44.1 kHz."""
    rng = np.random.Generator(np.random.PCG64(3212))
    return sorted(int(round(x)) for x in np.exp(rng.uniform(np.log(40), np.log(1200), size=32)))


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def setup(dev):
    from enhancer import Enhancer
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "config.json"), "w") as fh:
        json.dump(CONFIG, fh)
    torch.save({"generator": GC.nsf_state_dict(CONFIG, seed=91)}, os.path.join(tmp, "model"))
    enh = Enhancer("nsf-hifigan", os.path.join(tmp, "model"), device=dev)
    rng = np.random.default_rng(9)
    frames = slice_frames()
    rows = [torch.from_numpy((0.1 * rng.standard_normal(n * HOP)).astype(np.float32)).to(dev) for n in frames]
    f0 = [torch.from_numpy((220.0 * 2.0 ** (0.3 * np.sin(np.arange(n) / 50.0))).astype(np.float32)).to(dev) for n in frames]
    return enh, frames, rows, f0, torch.zeros(9, device=dev)


def loop_only():
    """The per-slice loop of the tree on sys.path as one JSON line."""
    enh, frames, rows, f0, ri = setup(torch.device("cuda:0"))

    def loop():
        for r, f in zip(rows, f0):
            enh.enhance(r[None], SR, f[None, :, None], HOP, rand_ini=ri)

    print("LOOP_JSON " + json.dumps(timed(loop)), flush=True)


def child(tree):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-only", "--tree", os.path.abspath(tree)],
                       capture_output=True, text=True, timeout=300, cwd=os.path.abspath(tree))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LOOP_JSON ")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"the per-slice loop of {tree} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1][len("LOOP_JSON "):])


def main():
    a = ARGS
    if a.loop_only:
        return loop_only()
    from infer_offline import group_segments
    from sharding import stack_rows
    loops = {"parent_tree": [], "this_tree": []}
    for _ in range(a.rounds):          # alternating order, fresh processes
        if a.baseline_tree:
            loops["parent_tree"].append(child(a.baseline_tree))
        loops["this_tree"].append(child(ROOT))
    dev = torch.device("cuda:0")
    enh, frames, rows, f0, ri = setup(dev)
    lengths = [int(r.numel()) for r in rows]
    result = {"device": torch.cuda.get_device_name(0), "frames": frames, "samples": lengths, "warmup": WARMUP, "runs": RUNS,
              "per_slice_loop": loops, "ragged": {}}
    base = loops["parent_tree"] or loops["this_tree"]
    loop_ms = float(np.median([r["median_ms"] for r in base]))
    result["per_slice_loop_median_ms"] = {k: float(np.median([r["median_ms"] for r in v])) for k, v in loops.items() if v}
    for budget in BUDGETS:
        groups = group_segments(lengths, budget)
        batches = []
        for g in groups:
            wav, counts = stack_rows([rows[i] for i in g])
            track, n_f0 = stack_rows([f0[i] for i in g])
            batches.append((wav, track[:, :, None], counts, n_f0))
        padded = sum(len(g) * max(lengths[i] for i in g) for g in groups)

        def run():
            for wav, track, counts, n_f0 in batches:
                enh.enhance_batch(wav, SR, track, HOP, counts, rand_ini=ri, n_f0=n_f0)

        rec = {"groups": len(groups), "padded_to_real_samples": padded / sum(lengths), "times": timed(run)}
        rec["loop_over_ragged"] = loop_ms / rec["times"]["median_ms"]
        result["ragged"][str(budget)] = rec
        print(budget, json.dumps(rec), flush=True)
    print(json.dumps(result["per_slice_loop"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
