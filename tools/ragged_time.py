"""Ragged batches against the per-slice loop: 32 slices, log-uniform in 40..1200 frames (0.5 - 14 s, what a silence slicer
with the reference's defaults leaves), CombSub and CombSubFast, one GPU session.

  (a) the per-slice batch-1 loop, timed on the build of ANOTHER checkout given with --baseline-tree (the commit before
      ragged batches existed, built with its own hipddsp/build.py) in a child process of the same session, so that a cost
      the feature added to the rectangular kernels cannot cancel out of (a)/(b); the same loop on this build is reported
      beside it (`a_this_build`).  Without --baseline-tree only the latter is measured and the ratios are marked so;
  (b) one ragged forward of all 32 slices;
  (c) the grouping of `infer_offline.render(batch_frames=)` at a few bounds: one ragged forward per group.
HIP events around the whole set of forwards, 3 warm-up rounds, median of 15; in-kernel noise.  Writes
profiles/ragged_time.json with the times, (a)/(b), (a)/(c) and each grouping's padded-to-real frame ratio.

    python tools/ragged_time.py --baseline-tree /path/to/built/parent/checkout [--out profiles/ragged_time.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ap = argparse.ArgumentParser()
_ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_time.json"))
_ap.add_argument("--baseline-tree", default=None, help="a built checkout whose per-slice loop is leg (a)")
_ap.add_argument("--loop-only", action="store_true", help="(child process) time the per-slice loop of --tree, print JSON")
_ap.add_argument("--tree", default=ROOT)
ARGS = _ap.parse_args()
sys.path[:0] = [ARGS.tree, os.path.join(ARGS.tree, "ddsp-svc-official_amd")]

import synthetic  # noqa: E402

WARMUP, ROUNDS = 3, 15


def slice_lengths():
    rng = np.random.Generator(np.random.PCG64(3212))
    return sorted(int(round(x)) for x in np.exp(rng.uniform(np.log(40), np.log(1200), size=32)))


def make_rows(lengths, dev):
    rows = []
    for i, n in enumerate(lengths):
        d = synthetic.make_inputs(100 + i, 1, n, with_noise=False)
        rows.append({k: v.to(dev) for k, v in d.items()})
    return rows


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def loop_only():
    """The per-slice loop of the tree on sys.path: {model: timing} as one JSON line."""
    dev = torch.device("cuda:0")
    lengths = slice_lengths()
    out = {}
    for name in ("CombSub", "CombSubFast"):
        model, cfg = synthetic.build_model(name, seed=7, device=dev)
        rows = make_rows(lengths, dev)
        spk = rows[0]["spk_id"]

        def loop():
            for r in rows:
                model(r["units"], r["f0"], r["volume"], spk, noise_seed=1)

        with torch.no_grad():
            out[name] = timed(loop)
    print("LOOP_JSON " + json.dumps(out), flush=True)


def main():
    a = ARGS
    if a.loop_only:
        return loop_only()
    from infer_offline import group_segments
    from sharding import stack_rows
    baseline = None
    if a.baseline_tree:
        # a fresh child process: its own interpreter, its own copy of the library, the GPU of this session
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-only", "--tree", os.path.abspath(a.baseline_tree)],
                           capture_output=True, text=True, timeout=600, cwd=os.path.abspath(a.baseline_tree))
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LOOP_JSON ")]
        if r.returncode != 0 or not lines:
            raise RuntimeError(f"baseline loop failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        baseline = json.loads(lines[-1][len("LOOP_JSON "):])
    dev = torch.device("cuda:0")
    lengths = slice_lengths()
    real = sum(lengths)
    result = {"device": torch.cuda.get_device_name(0), "lengths": lengths, "real_frames": real, "warmup": WARMUP,
              "rounds": ROUNDS, "a_is": "baseline tree" if baseline else "this build (no --baseline-tree)", "models": {}}
    for name in ("CombSub", "CombSubFast"):
        model, cfg = synthetic.build_model(name, seed=7, device=dev)
        rows = make_rows(lengths, dev)
        spk = rows[0]["spk_id"]

        def batch(group):
            u, counts = stack_rows([rows[i]["units"][0] for i in group])
            f, _ = stack_rows([rows[i]["f0"][0] for i in group])
            v, _ = stack_rows([rows[i]["volume"][0] for i in group])
            return u, f, v, counts

        def loop():
            for r in rows:
                model(r["units"], r["f0"], r["volume"], spk, noise_seed=1)

        def grouped(batches):
            def run():
                for u, f, v, counts in batches:
                    model(u, f, v, spk, noise_seed=1, n_frames=counts)
            return run

        with torch.no_grad():
            rec = {"a_this_build": timed(loop)}
            rec["a_per_slice_loop"] = baseline[name] if baseline else rec["a_this_build"]
            one = [batch(list(range(len(lengths))))]
            rec["b_one_ragged_forward"] = dict(timed(grouped(one)), padded_to_real=len(lengths) * max(lengths) / real)
            rec["c_batch_frames"] = {}
            for bound in (1024, 2048, 4096, 8192, 16384):
                groups = group_segments(lengths, bound)
                padded = sum(len(g) * max(lengths[i] for i in g) for g in groups)
                rec["c_batch_frames"][str(bound)] = dict(timed(grouped([batch(g) for g in groups])), groups=len(groups),
                                                         padded_to_real=padded / real)
        a_ms = rec["a_per_slice_loop"]["median_ms"]
        rec["a_over_b"] = a_ms / rec["b_one_ragged_forward"]["median_ms"]
        for k, v in rec["c_batch_frames"].items():
            v["a_over_c"] = a_ms / v["median_ms"]
        result["models"][name] = rec
        print(name, json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
