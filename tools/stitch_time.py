"""Timing of the end of an offline conversion on the file of the slicer's DESIGN entry: 5 minutes at 44.1 kHz (13.2 M samples)
in about 100 rendered pieces, a third of them behind a gap, a third abutting, a third overlapping the one before by 64 to 2048
samples.  Synthetic fp32 pieces on the device, no model.

    python tools/stitch_time.py [--iters N] [--host-iters H] [--warmup W] [--seconds S] [--pieces P] [--out file.json]

Two legs of the stitch, in one session, each on the wall clock around work that ends with the result on the host:
  host    the tail of `infer_offline.render`: per piece `.cpu().numpy()` (a synchronisation each), then `np.append` twice or
          `cross_fade` - each copies the whole float64 result so far;
  device  `infer_offline.stitch` (one table upload, one `ddsp_stitch` launch) and one `.cpu()` of the fp64 result.
The device leg is also bracketed by device events without the read-back (the launch alone), with its rate against 12 bytes
per output sample (4 read, 8 written).  Both legs give the same array; the script asserts it.
Two legs of the gate over the same slices (frames of 512 samples):
  per slice  what `render` does: `volume_mask(volume)` - a whole-file `ones`, gated - cut to the slice and multiplied in;
  rows       one `ddsp_volume_gate_rows` over the padded group tensor.
Median and p99 over the repeats after the warm-up calls."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ddsp-svc-official_amd")):
    sys.path.insert(0, p)

import hipddsp  # noqa: E402
import infer_offline  # noqa: E402

SR, HOP = 44100, 512


def layout(seconds, n_pieces, seed=11):
    """-> (start frames, frame counts, start samples, sample counts): pieces of 0.5 to 1.5 times the mean length in whole
    frames; piece i starts behind a gap of 1 to 8 frames (i % 3 == 0), where the last ended (1), or 64 to 2048 samples before
    that (2) - the sample starts are what the stitch sees, the frame starts (no overlap) what the gate sees."""
    rng = np.random.Generator(np.random.PCG64(seed))
    mean = seconds * SR / HOP / n_pieces
    frames = [max(8, int(mean * rng.uniform(0.5, 1.5))) for _ in range(n_pieces)]
    f_start, s_start, f_cur, s_cur = [], [], 0, 0
    for i, n in enumerate(frames):
        if i % 3 == 0:
            gap = int(rng.integers(1, 9))
            f_cur, s_cur = f_cur + gap, s_cur + gap * HOP
        over = int(rng.integers(64, 2049)) if i % 3 == 2 else 0
        f_start.append(f_cur)
        s_start.append(s_cur - over)
        f_cur, s_cur = f_cur + n, s_cur - over + n * HOP
    return f_start, frames, s_start, [n * HOP for n in frames]


def wall(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.percentile(ms, 99))


def events(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.percentile(ms, 99))


def host_stitch(pieces, starts):
    """The tail of `render` (main.py:165-173) at sr_o == sr with the start given in samples."""
    result, current = np.zeros(0), 0
    for x, at in zip(pieces, starts):
        out = x.squeeze().cpu().numpy()
        silent = at - current
        if silent >= 0:
            result = np.append(result, np.zeros(silent))
            result = np.append(result, out)
        else:
            result = infer_offline.cross_fade(result, out, current + silent)
        current = current + silent + len(out)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--pieces", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = hipddsp.context_for(dev)
    f_start, frames, s_start, lengths = layout(a.seconds, a.pieces)
    gen = torch.Generator(device=dev).manual_seed(5)
    pieces = [torch.rand(1, n, device=dev, generator=gen) - 0.5 for n in lengths]
    plan = infer_offline.stitch_plan(s_start, lengths, 1, SR, SR)
    total = plan[2]

    host_ms, host99 = wall(lambda: host_stitch(pieces, s_start), a.host_iters, 1)
    dev_ms, dev99 = wall(lambda: infer_offline.stitch(pieces, plan).cpu(), a.iters, a.warmup)
    launch_ms, launch99 = events(lambda: infer_offline.stitch(pieces, plan), a.iters, a.warmup)
    same = bool(np.array_equal(host_stitch(pieces, s_start), infer_offline.stitch(pieces, plan).cpu().numpy()))
    assert same, "the device stitch differs from the host loop"

    # the gate: the same slices as frames of one file's volume
    Fr = f_start[-1] + frames[-1] + 4
    volume = torch.rand(1, Fr, device=dev, generator=gen) * 0.3
    volume[0, Fr // 3:Fr // 3 + 200] = 0.0
    group = torch.rand(len(frames), max(lengths), device=dev, generator=gen)
    starts_dev, counts_dev = ctx.ragged_counts(f_start), ctx.ragged_counts(frames)

    def per_slice():
        for x, s, n in zip(pieces, f_start, frames):
            x *= infer_offline.volume_mask(volume, -60, HOP)[:, s * HOP:(s + n) * HOP]

    slice_ms, slice99 = wall(per_slice, max(3, a.iters // 4), 1)
    rows_ms, rows99 = wall(lambda: ctx.volume_gate_rows_(group, volume[0], starts_dev, counts_dev, -60, HOP), a.iters, a.warmup)
    ctx.poll_error()

    row = {"device": torch.cuda.get_device_name(0), "seconds": total / SR, "samples": total, "pieces": len(pieces),
           "gaps": sum(1 for i in range(len(pieces)) if i % 3 == 0), "cross_fades": sum(1 for f in plan[1] if f),
           "same_array_as_host_loop": same,
           "host_loop_wall_ms": host_ms, "host_loop_wall_p99_ms": host99, "host_iters": a.host_iters,
           "stitch_and_one_readback_wall_ms": dev_ms, "stitch_and_one_readback_wall_p99_ms": dev99,
           "stitch_launch_ms": launch_ms, "stitch_launch_p99_ms": launch99,
           "stitch_GBps_of_12_bytes_per_sample": 12.0 * total / (launch_ms * 1e-3) / 1e9,
           "host_over_device": host_ms / dev_ms,
           "gate_per_slice_wall_ms": slice_ms, "gate_per_slice_wall_p99_ms": slice99,
           "gate_rows_wall_ms": rows_ms, "gate_rows_wall_p99_ms": rows99, "gate_per_slice_over_rows": slice_ms / rows_ms,
           "iters": a.iters, "warmup": a.warmup}
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(row, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
