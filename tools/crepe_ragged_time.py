"""Ragged CREPE and the ragged dataset analysis against the per-file loop: 32 utterances of 0.6 - 13 s at 44.1 kHz, the 'full'
network (fixture weight fill), the context's default product mode, one GPU session.

  (a) the per-file loop, `F0_Extractor.extract(x_i)` 32 times at batch 1, and `preprocess.analyse_batch(batch_samples=None)`
      where the tree has it: what the reference's preprocess.py does.  Run in child processes on --baseline-tree (a built
      checkout of the parent commit, which has no ragged CREPE) and on this tree, alternating;
  (b) `F0_Extractor.extract(x_group, n_samples=)` once per group of `infer_offline.group_segments` at several
      `batch_samples` budgets, and for all files in one group;
  (c) the whole `preprocess.analyse_batch(batch_samples=)` (volume, HuBERT-Soft units, f0, copies to the host) at the same
      budgets.
Device events around each whole set of calls for (a) and (b), wall time around (c) (it ends on the host); 2 warm-up rounds,
6 timed: mean and min.  Reports, per budget, the share of PACKED frames (what ragged CREPE computes) among the PADDED
frames (what a rectangular batch of the same groups would compute).  Writes profiles/crepe_ragged_time.json.

    python tools/crepe_ragged_time.py [--baseline-tree /path/to/built/parent/checkout] [--out profiles/crepe_ragged_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ap = argparse.ArgumentParser()
_ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crepe_ragged_time.json"))
_ap.add_argument("--baseline-tree", default=None, help="a built checkout of the parent commit for the per-file loop")
_ap.add_argument("--loop-only", action="store_true", help="(child process) time (a) of --tree, print JSON")
_ap.add_argument("--tree", default=ROOT)
_ap.add_argument("--rounds", type=int, default=1, help="child processes per tree, alternating")
ARGS = _ap.parse_args()
sys.path[:0] = [ARGS.tree, os.path.join(ARGS.tree, "ddsp-svc-official_amd"), os.path.join(ROOT, "tests")]

import crepe_cases as CC  # noqa: E402
import hubert_cases as HC  # noqa: E402

SR, HOP = 44100, 512
WARMUP, RUNS = 2, 6
BUDGETS = [600000, 1200000, 2400000, 4800000, 9600000]


def lengths_44k():
    rng = np.random.Generator(np.random.PCG64(4421))
    return sorted(int(round(SR * s)) for s in np.exp(rng.uniform(np.log(0.6), np.log(13.0), size=32)))


def timed(fn, wall=False):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        if wall:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
    return {"mean_ms": float(np.mean(ms)), "min_ms": float(min(ms))}


def setup(dev):
    from ddsp.crepe import Crepe
    from ddsp.hubert import HubertSoft
    from ddsp.vocoder import Audio2HubertSoft, F0_Extractor, Units_Encoder, Volume_Extractor
    crepe = Crepe("full")
    crepe.load_state_dict(CC.fill("full"))
    f0x = F0_Extractor("crepe", SR, HOP, 65, 800, crepe_ckpt=crepe, device=dev)
    a2h = Audio2HubertSoft.__new__(Audio2HubertSoft)      # (the constructor reads a checkpoint file: the fill instead)
    torch.nn.Module.__init__(a2h)
    a2h.hubert = HubertSoft()
    a2h.hubert.load_state_dict(HC.fill({k: tuple(v.shape) for k, v in a2h.hubert.state_dict().items()}), strict=True)
    a2h.hubert.to(dev).eval()
    enc = Units_Encoder.__new__(Units_Encoder)
    enc.device, enc.model, enc.encoder_sample_rate, enc.encoder_hop_size = dev, a2h.eval(), 16000, 320
    rng = np.random.default_rng(9)
    waves = []
    for i, n in enumerate(lengths_44k()):
        t = np.arange(n) / SR
        waves.append((0.3 * np.sin(2 * np.pi * (110 + 9 * i) * t * (1 + 0.02 * t)) + 0.01 * rng.standard_normal(n)).astype(np.float32))
    return f0x, Volume_Extractor(HOP, device=dev), enc, waves


def loop_only():
    """(a) of the tree on sys.path as one JSON line."""
    dev = torch.device("cuda:0")
    f0x, vol, enc, waves = setup(dev)
    rows = [torch.from_numpy(w).to(dev)[None] for w in waves]

    def f0_loop():
        for x in rows:
            f0x.extract(x, uv_interp=False)

    out = {"f0_per_file_loop": timed(f0_loop)}
    try:
        import preprocess as PP
        out["analyse_per_file_loop"] = timed(lambda: PP.analyse_batch(waves, f0x, vol, enc, SR, HOP), wall=True)
    except ImportError:
        # the parent commit has no preprocess module: its per-file analysis is the three calls and the copies to the host
        def analyse():
            for x in rows:
                vol.extract(x).cpu()
                enc.encode(x, SR, HOP).cpu()
                f0x.extract(x, uv_interp=False).cpu()
        out["analyse_per_file_loop"] = timed(analyse, wall=True)
    print("LOOP_JSON " + json.dumps(out), flush=True)


def child(tree):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-only", "--tree", os.path.abspath(tree)],
                       capture_output=True, text=True, timeout=900, cwd=os.path.abspath(tree))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LOOP_JSON ")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"per-file timing of {tree} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1][len("LOOP_JSON "):])


def main():
    a = ARGS
    if a.loop_only:
        return loop_only()
    import hipddsp
    import preprocess as PP
    from infer_offline import group_segments
    from sharding import stack_rows
    loops = {"this_tree": [], "baseline_tree": []}
    for _ in range(a.rounds):          # alternating order, fresh processes
        if a.baseline_tree:
            loops["baseline_tree"].append(child(a.baseline_tree))
        loops["this_tree"].append(child(ROOT))
    dev = torch.device("cuda:0")
    f0x, vol, enc, waves = setup(dev)
    lengths = [len(w) for w in waves]
    lib = hipddsp.load_library()
    frames = [hipddsp.crepe_frames(int(lib.ddsp_resample_length(n, SR, 16000))) for n in lengths]
    base = loops["baseline_tree"] or loops["this_tree"]
    loop_ms = {k: float(np.mean([r[k]["mean_ms"] for r in base])) for k in ("f0_per_file_loop", "analyse_per_file_loop")}
    result = {"device": torch.cuda.get_device_name(0), "network": "full", "samples_44k": lengths, "crepe_frames": frames,
              "warmup": WARMUP, "runs": RUNS, "per_file_loop": loops, "per_file_loop_mean_ms": loop_ms,
              "per_file_loop_from": "baseline_tree" if loops["baseline_tree"] else "this_tree", "ragged": {}}
    rows = [torch.from_numpy(w).to(dev) for w in waves]
    for budget in BUDGETS + [len(lengths) * max(lengths)]:
        groups = group_segments(lengths, budget)
        batches = [stack_rows([rows[i] for i in g]) for g in groups]
        padded = sum(len(g) * max(frames[i] for i in g) for g in groups)

        def f0_run():
            for x, counts in batches:
                f0x.extract(x, uv_interp=False, n_samples=counts)

        rec = {"groups": len(groups), "packed_frames": sum(frames), "padded_frames": padded,
               "packed_over_padded": sum(frames) / padded, "f0": timed(f0_run),
               "analyse_batch": timed(lambda: PP.analyse_batch(waves, f0x, vol, enc, SR, HOP, batch_samples=budget), wall=True)}
        rec["f0_loop_over_ragged"] = loop_ms["f0_per_file_loop"] / rec["f0"]["mean_ms"]
        rec["analyse_loop_over_ragged"] = loop_ms["analyse_per_file_loop"] / rec["analyse_batch"]["mean_ms"]
        result["ragged"][str(budget)] = rec
        print(budget, json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
