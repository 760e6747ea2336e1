"""Ragged HuBERT-Soft against the per-slice loop: the units of 32 slices of 0.5 - 14 s (the slice set of
tools/ragged_time.py, as 16 kHz audio), fixture weight fill, both product modes, one GPU session.

  (a) the per-slice loop, `units(wav_i)` 32 times: what `convert_batched(units_batch_samples=None)` does;
  (b) ragged groups, `units(wav_group, n_samples=)` once per group of `infer_offline.group_segments` over the sample
      lengths, at several `units_batch_samples` (here in 16 kHz samples) and for all slices in one group;
  (c) the rectangular GUI-window call (72000 samples, 225 frames).
(a) and (c) run in child processes, one per tree, alternating between this tree and - with --baseline-tree, a built checkout
of the commit before the ragged encoder - that one, so that a cost the feature added to the rectangular kernels shows as a
difference between two builds measured minutes apart on one device.
Device events around each whole set of calls, 5 warm-up rounds, 30 timed: mean and p99.  Writes
profiles/hubert_ragged_time.json with the times, (a)/(b) and each grouping's share of padded frames.

    python tools/hubert_ragged_time.py [--baseline-tree /path/to/built/parent/checkout] [--out profiles/hubert_ragged_time.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ap = argparse.ArgumentParser()
_ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hubert_ragged_time.json"))
_ap.add_argument("--baseline-tree", default=None, help="a built checkout whose rectangular calls are compared with this one's")
_ap.add_argument("--rect-only", action="store_true", help="(child process) time (a) and (c) of --tree, print JSON")
_ap.add_argument("--tree", default=ROOT)
_ap.add_argument("--rounds", type=int, default=2, help="child processes per tree, alternating")
ARGS = _ap.parse_args()
sys.path[:0] = [ARGS.tree, os.path.join(ARGS.tree, "ddsp-svc-official_amd"), os.path.join(ROOT, "tests")]

import hubert_cases as HC  # noqa: E402

WARMUP, RUNS = 5, 30
BUDGETS = [125000, 250000, 500000, 1000000, 2000000]
MODES = ("fp32", "split")


def slice_samples():
    """The 32 slice lengths of tools/ragged_time.py (frames of 512 samples at 44.1 kHz) as 16 kHz sample counts."""
    rng = np.random.Generator(np.random.PCG64(3212))
    frames = sorted(int(round(x)) for x in np.exp(rng.uniform(np.log(40), np.log(1200), size=32)))
    return [int(round(n * 512 / 44100 * 16000)) for n in frames]


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
    return {"mean_ms": float(np.mean(ms)), "p99_ms": float(np.percentile(ms, 99)), "min_ms": float(min(ms))}


def setup(dev):
    import hipddsp
    from ddsp.hubert import HubertSoft
    m = HubertSoft()
    m.load_state_dict(HC.fill({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
    m = m.to(dev).eval()
    rng = np.random.default_rng(9)
    rows = [torch.from_numpy((0.1 * rng.standard_normal(n)).astype(np.float32)).to(dev) for n in slice_samples()]
    return hipddsp, hipddsp.context_for(dev), m, rows


def each_mode(hipddsp, ctx, fn):
    out = {}
    prev = ctx.math
    for mode in MODES:
        ctx.set_math(hipddsp.MATH_FP32 if mode == "fp32" else hipddsp.MATH_SPLIT_BF16)
        out[mode] = timed(fn)
    ctx.set_math(prev)
    return out


def rect_only():
    """(a) and (c) of the tree on sys.path as one JSON line."""
    dev = torch.device("cuda:0")
    hipddsp, ctx, m, rows = setup(dev)
    wavs = [r[None, None] for r in rows]
    gui = HC.audio("gui").unsqueeze(1).to(dev)

    def loop():
        for w in wavs:
            m.units(w)

    out = {"per_slice_loop": each_mode(hipddsp, ctx, loop), "gui_window": each_mode(hipddsp, ctx, lambda: m.units(gui))}
    print("RECT_JSON " + json.dumps(out), flush=True)


def child(tree):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rect-only", "--tree", os.path.abspath(tree)],
                       capture_output=True, text=True, timeout=600, cwd=os.path.abspath(tree))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RECT_JSON ")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"rectangular timing of {tree} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1][len("RECT_JSON "):])


def main():
    a = ARGS
    if a.rect_only:
        return rect_only()
    from infer_offline import group_segments
    from sharding import stack_rows
    rect = {"this_tree": [], "baseline_tree": []}
    for _ in range(a.rounds):          # alternating order, fresh processes
        if a.baseline_tree:
            rect["baseline_tree"].append(child(a.baseline_tree))
        rect["this_tree"].append(child(ROOT))
    dev = torch.device("cuda:0")
    hipddsp, ctx, m, rows = setup(dev)
    lengths = [int(r.numel()) for r in rows]
    frames = [hipddsp.hubert_frames(n) for n in lengths]
    result = {"device": torch.cuda.get_device_name(0), "samples_16k": lengths, "frames": frames, "warmup": WARMUP, "runs": RUNS,
              "rectangular": rect, "ragged": {}}
    loop_ms = {mode: float(np.mean([r["per_slice_loop"][mode]["mean_ms"] for r in rect["this_tree"]])) for mode in MODES}
    result["per_slice_loop_mean_ms"] = loop_ms
    for budget in BUDGETS + [len(lengths) * max(lengths)]:
        groups = group_segments(lengths, budget)
        batches = []
        for g in groups:
            wav, counts = stack_rows([rows[i] for i in g])
            batches.append((wav[:, None], m.counts(counts, len(g), wav.shape[1], dev)))   # uploaded once, outside the timing
        padded = sum(len(g) * hipddsp.hubert_frames(max(lengths[i] for i in g)) for g in groups)

        def run():
            for wav, counts in batches:
                m.units(wav, n_samples=counts)

        rec = {"groups": len(groups), "padded_frame_share": 1.0 - sum(frames) / padded, "times": each_mode(hipddsp, ctx, run)}
        rec["loop_over_ragged"] = {mode: loop_ms[mode] / rec["times"][mode]["mean_ms"] for mode in MODES}
        result["ragged"][str(budget)] = rec
        print(budget, json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
