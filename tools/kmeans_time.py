"""What the unit index reduction costs: one `Context.units_kmeans_assign_` and one `units_kmeans_update_` call against the same
steps written in torch, and `UnitIndex.reduce` end to end.

Shapes (N, K, C) = (200 000, 10 000, 256) and (200 000, 10 000, 768), normal entries, the strided initial centres.  The torch form
of the assignment is a chunked `cnrm - 2 x @ cen.T` (chunks of `--chunk` entries, so the score matrix stays at chunk x K) and
`argmin`; of the update, `index_add_` for the sums (fp32, order-dependent: the yardstick for time, not for bits) and `bincount`.
The update works in place, so the centres are put back in front of every timed call, outside its event pair.
Both forms run in ONE process and ALTERNATE call by call (HIP events around each; a warm-up first), so clocks and other tenants
move both alike; the median and the fastest of `--repeats` calls are written, with the assignment's FLOP/s against the fp32
matrix peak (`--peak-tflops`).  `reduce` is timed once per shape on the wall clock, upload and read-back included.

    python tools/kmeans_time.py [--out profiles/kmeans_time.json] [--repeats 10] [--iters 10] [--shapes 256,768] [--reduce-shapes 256,768]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ddsp-svc-official_amd"))

N, K = 200_000, 10_000


def torch_assign(vec, cen, cnrm, chunk):
    import torch
    out = torch.empty(vec.shape[0], dtype=torch.int64, device=vec.device)
    for a in range(0, vec.shape[0], chunk):
        out[a:a + chunk] = torch.argmin(cnrm[None, :] - 2.0 * (vec[a:a + chunk] @ cen.T), dim=1)
    return out


def torch_update(vec, assign, cen):
    import torch
    sums = torch.zeros_like(cen).index_add_(0, assign, vec)
    count = torch.bincount(assign, minlength=cen.shape[0])
    return torch.where(count[:, None] > 0, sums / count.clamp(min=1)[:, None], cen), count


def time_calls(a, repeats, warmup):
    """Alternate the forms; -> {name: [ms]}.  A form is fn or (prepare, fn): prepare runs in front of the timed pair."""
    import torch
    out = {name: [] for name in a}
    for i in range(warmup + repeats):
        for name, fn in a.items():
            if isinstance(fn, tuple):
                fn[0]()
                fn = fn[1]
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            if i >= warmup:
                out[name].append(start.elapsed_time(stop))
    return out


def steps(C, repeats, warmup, chunk, peak):
    import numpy as np
    import torch

    import hipddsp
    from infer_offline import UnitIndex
    dev = torch.device("cuda:0")
    ctx = hipddsp.context_for(dev)
    host = torch.randn(N, C, generator=torch.Generator().manual_seed(N + C))
    vec = host.to(dev)
    start = vec[(torch.arange(K, dtype=torch.int64, device=dev) * N) // K].contiguous()
    cnrm = ctx.units_index_norms(start)
    shift = UnitIndex.fixed_shift(host)
    assign = torch.full((N,), -1, dtype=torch.int32, device=dev)
    moved = torch.zeros(1, dtype=torch.int32, device=dev)
    count = torch.empty(K, dtype=torch.int32, device=dev)
    ws = torch.empty(K * C, dtype=torch.int64, device=dev)
    cen = start.clone()
    ctx.units_kmeans_assign_(vec, start, cnrm, assign, moved)                    # the assignment both updates start from
    ids = assign.long()
    t = time_calls({"assign_kernel": lambda: ctx.units_kmeans_assign_(vec, start, cnrm, assign, moved),
                    "assign_torch": lambda: torch_assign(vec, start, cnrm, chunk),
                    "update_kernel": (lambda: cen.copy_(start), lambda: ctx.units_kmeans_update_(vec, assign, cen, count, shift, ws)),
                    "update_torch": lambda: torch_update(vec, ids, start)}, repeats, warmup)
    torch.cuda.synchronize()
    ctx.poll_error()
    differ = int((torch_assign(vec, start, cnrm, chunk) != assign.long()).sum())
    mean_diff = float((torch_update(vec, ids, start)[0] - cen).abs().max())
    flop = 2.0 * N * K * C
    row = {"N": N, "K": K, "C": C, "repeats": repeats, "warmup": warmup, "torch_chunk": chunk,
           **{f"{name}_median_ms": float(np.median(v)) for name, v in t.items()},
           **{f"{name}_min_ms": float(np.min(v)) for name, v in t.items()},
           "assign_flop": flop, "assign_kernel_tflops": flop / (float(np.median(t["assign_kernel"])) * 1e-3) / 1e12,
           "assign_torch_tflops": flop / (float(np.median(t["assign_torch"])) * 1e-3) / 1e12, "fp32_matrix_peak_tflops": peak,
           "assign_kernel_of_peak": flop / (float(np.median(t["assign_kernel"])) * 1e-3) / 1e12 / peak,
           "ids_that_differ_from_torch": differ, "max_abs_diff_of_the_means_to_torch": mean_diff}
    print(json.dumps(row), flush=True)
    return row


def whole(C, iters):
    import torch

    from infer_offline import UnitIndex
    index = UnitIndex(torch.randn(N, C, generator=torch.Generator().manual_seed(N + C)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out, rep = index.reduce(K, iters=iters, device="cuda:0", report=True)
    row = {"N": N, "K": K, "C": C, "iters": iters, "reduce_wall_s": time.perf_counter() - t0, "centres_out": len(out),
           "dropped": rep["dropped"], "moved": rep["moved"]}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_time.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=8192, help="entries of one torch score matrix")
    ap.add_argument("--shapes", default="256,768", help="the widths C whose steps are timed")
    ap.add_argument("--reduce-shapes", default="256,768", help="the widths C whose whole reduction is timed ('' for none)")
    ap.add_argument("--peak-tflops", type=float, default=157.3, help="the fp32 matrix peak the assignment is quoted against")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_time needs a HIP device")
    widths = lambda s: [int(c) for c in s.split(",") if c]  # noqa: E731
    doc = {"what": "one units_kmeans_assign_ / units_kmeans_update_ call against a chunked matmul + argmin / index_add_ in torch, "
                   "alternating in one process (HIP events, median and fastest of `repeats`); reduce: wall clock of UnitIndex.reduce",
           "device": torch.cuda.get_device_name(0), "steps": [], "reduce": []}

    def write():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    for C in widths(a.shapes):
        doc["steps"].append(steps(C, a.repeats, a.warmup, a.chunk, a.peak_tflops))
        torch.cuda.empty_cache()
        write()
    for C in widths(a.reduce_shapes):
        doc["reduce"].append(whole(C, a.iters))
        write()


if __name__ == "__main__":
    main()
