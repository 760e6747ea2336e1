"""Timing of the silence slicer (`ddsp_slicer` behind `slicer.Slicer` / `infer_offline.split`) on a 5-minute signal at
44.1 kHz with the reference's defaults (hop 882, window 3528, about 15 000 frames): tone bursts of 0.5 to 6 s with noise floors
of 0.2 to 2 s between them, seeded.

    python tools/slicer_time.py [--iters N] [--warmup W] [--seconds S] [--out file.json]

Device events bracket every call after W warm-up calls; mean and p99 of N calls.  One `ctx.slicer` call launches the two
kernels back to back, so they are told apart by a second series with min_length above the sample count: the tagging kernel
then takes the reference's early return and only the frame-RMS kernel does work; the tagging kernel's time is the difference
of the two series.  The RMS kernel's rate is stated against 4 * T bytes, the audio read once.  `split` is timed end to end
on the wall clock with its one read-back, from a device tensor and from a numpy array (which adds the upload).  Beside it the
host path a user has without the package's slicer: the numpy restatement of tests/slicer_cases.py (fp32 RMS and the state
machine) in the same process."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ddsp-svc-official_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import hipddsp  # noqa: E402
import infer_offline  # noqa: E402
import slicer_cases as SC  # noqa: E402
from slicer import Slicer  # noqa: E402
from crepe_time import timed  # noqa: E402

SR = 44100


def signal(seconds, seed=7):
    rng = np.random.Generator(np.random.PCG64(seed))
    T = int(seconds * SR)
    x = np.empty(T, dtype=np.float32)
    t, voiced = 0, True
    while t < T:
        n = min(T - t, int(SR * (rng.uniform(0.5, 6.0) if voiced else rng.uniform(0.2, 2.0))))
        if voiced:
            x[t:t + n] = 0.3 * np.sin(2 * np.pi * 220.0 * np.arange(t, t + n) / SR)
        else:
            x[t:t + n] = 1e-4 * (0.5 + rng.random()) * rng.standard_normal(n)
        t, voiced = t + n, not voiced
    return x


def wall(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.mean(ms)), float(np.percentile(ms, 99))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = hipddsp.context_for(dev)
    x = signal(a.seconds)
    T = x.shape[0]
    s = Slicer(SR, device=dev)
    xd = torch.from_numpy(x).to(dev)[None]
    F = s.frames(T)
    out = ctx.slicer(xd, s.win_size, s.hop_size, s.threshold, s.min_length, s.min_interval, s.max_sil_kept)

    def call(min_length):
        return lambda: ctx.slicer(xd, s.win_size, s.hop_size, s.threshold, min_length, s.min_interval, s.max_sil_kept, out=out)

    both, both99 = timed(call(s.min_length), a.iters, a.warmup)
    chunks = int(out[1][0])
    rms_ms, rms99 = timed(call(T), a.iters, a.warmup)
    assert int(out[1][0]) == 1
    split_dev, split_dev99 = wall(lambda: infer_offline.split(xd[0], SR, 512.0), a.iters, a.warmup)
    split_np, split_np99 = wall(lambda: infer_offline.split(x, SR, 512.0), max(3, a.iters // 10), 1)
    ranges = infer_offline.split(xd[0], SR, 512.0)

    fr = SC.frames_of(dict(sr=SR))
    t0 = time.perf_counter()
    host_iters = 3
    for _ in range(host_iters):
        r = SC.rms(x, fr["win"], fr["hop"], "constant", np.float32)
        t1 = time.perf_counter()
        tagged = SC.tag(r, T, fr)
        host_tag_ms = (time.perf_counter() - t1) * 1e3
    host_ms = (time.perf_counter() - t0) * 1e3 / host_iters
    host_ranges = [(int(p), int(q)) for p, q, _ in tagged["chunks"] if p != q]
    row = {"device": torch.cuda.get_device_name(0), "seconds": T / SR, "samples": T, "frames": F, "hop": s.hop_size,
           "win": s.win_size, "chunks": chunks, "ranges": len(ranges), "same_ranges_as_host_restatement": ranges == host_ranges,
           "both_kernels_ms": both, "both_kernels_p99_ms": both99, "rms_kernel_ms": rms_ms, "rms_kernel_p99_ms": rms99,
           "tag_kernel_ms_by_difference": both - rms_ms, "rms_kernel_GBps_of_4T": 4.0 * T / (rms_ms * 1e-3) / 1e9,
           "split_from_device_tensor_wall_ms": split_dev, "split_from_device_tensor_wall_p99_ms": split_dev99,
           "split_from_numpy_wall_ms": split_np, "split_from_numpy_wall_p99_ms": split_np99,
           "host_numpy_restatement_ms": host_ms, "host_numpy_restatement_tagging_ms": host_tag_ms,
           "iters": a.iters, "warmup": a.warmup}
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(row, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
