"""What producing a training batch costs: `data_loaders.AudioDataset.batches` (one `ddsp_dataset_gather` launch per batch)
and, with --baseline, the reference's `cache_device='cuda'` loader restated here - per-item slices of device-cached tensors
(`data_loaders.py:98-146`) and the DataLoader's `torch.stack` collation - in the same process.  Run on the GPU box:
    python tools/dataset_time.py --baseline [--out profiles/dataset_time.json]
B = 32 crops of 2 s at 44.1 kHz / hop 512 with 256 unit channels, from a synthetic dataset of 256 files of 3 to 8 s.
Per producer: host time per batch (200 batches after warm-up, the clock read BEFORE the one synchronisation at the end),
device time per batch (events round the same window, so it includes whatever the device waited for the host), the host time
of a full `training.train_step` fed by the producer; for the kernel: time per launch (an event pair per launch, median) and
its bytes per second beside a `Tensor.copy_` of the same byte count measured the same way."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ddsp-svc-official_amd"))
import data_loaders as DL  # noqa: E402
import synthetic  # noqa: E402
import training  # noqa: E402
from ddsp.loss import RSSLoss  # noqa: E402

SR, HOP, SEC, C, B = 44100, 512, 2.0, 256, 32


def make_records(n_files, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    recs = []
    for i in range(n_files):
        n = int(rng.integers(3 * SR, 8 * SR))
        fr = n // HOP + 1
        recs.append({"name": f"{1 + i % 4}/f{i:04d}", "audio": (0.1 * rng.standard_normal(n, dtype=np.float32)),
                     "duration": n / SR, "spk_id": 1 + i % 4, "f0": rng.uniform(80, 600, fr).astype(np.float32),
                     "volume": rng.uniform(0, 0.3, fr).astype(np.float32),
                     "units": [rng.standard_normal((fr, C), dtype=np.float32)]})
    return recs


class BaselineLoader:
    """The reference's AudioDataset with cache_device='cuda' under DataLoader(shuffle=True, num_workers=0), restated."""

    def __init__(self, records, dev):
        self.buf = [{"audio": torch.from_numpy(r["audio"]).to(dev), "f0": torch.from_numpy(r["f0"]).unsqueeze(-1).to(dev),
                     "volume": torch.from_numpy(r["volume"]).to(dev), "units": [torch.from_numpy(u).to(dev) for u in r["units"]],
                     "spk_id": torch.LongTensor([r["spk_id"]]).to(dev), "duration": r["duration"]} for r in records]

    def item(self, i):
        d = self.buf[i]
        if d["duration"] < SEC + 0.1:
            return self.item((i + 1) % len(self.buf))
        units = d["units"][random.randint(0, len(d["units"]) - 1)]
        res = HOP / SR
        start = int(random.uniform(0, d["duration"] - SEC - 0.1) / res)
        n = int(SEC / res)
        return dict(audio=d["audio"][start * HOP:(start + n) * HOP], f0=d["f0"][start:start + n],
                    volume=d["volume"][start:start + n], units=units[start:start + n], spk_id=d["spk_id"])

    def batches(self, batch_size):
        order = torch.randperm(len(self.buf)).tolist()
        for s in range(0, len(order), batch_size):
            items = [self.item(i) for i in order[s:s + batch_size]]
            yield {k: torch.stack([it[k] for it in items]) for k in items[0]}


def forever(make_epoch):
    while True:
        yield from make_epoch()


def time_producer(it, n=200, warm=20):
    for _ in range(warm):
        next(it)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(n):
        b = next(it)
    t1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    assert b["units"].shape == (B, int(SEC / (HOP / SR)), C)
    return {"host_us_per_batch": 1e6 * (t1 - t0) / n, "device_us_per_batch": 1e3 * e0.elapsed_time(e1) / n}


def per_launch_us(fn, n=200, warm=20):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(1e3 * a.elapsed_time(b) for a, b in ev)
    return {"median_us": ts[n // 2], "p10_us": ts[n // 10], "p90_us": ts[9 * n // 10]}


def time_train(it, model, opt, crit, bucket, n=30, warm=5):
    def step():
        return training.train_step(model, opt, crit, next(it), scales=[300, 777, 1200, 2000], bucket=bucket)
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return {"host_ms_per_step": 1e3 * (t1 - t0) / n, "wall_ms_per_step": 1e3 * (t2 - t0) / n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", action="store_true", help="also time the restated reference loader")
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("dataset_time needs a HIP device: a CPU run gives no time")
    dev = torch.device("cuda:0")
    recs = make_records(args.files)
    ds = DL.AudioDataset(None, SEC, HOP, SR, n_spk=4, n_aunit=0, device=dev, records=recs)
    Fr = ds.crop
    res = {"device": torch.cuda.get_device_name(0), "B": B, "frames": Fr, "hop": HOP, "n_unit": C, "files": args.files,
           "batches_timed": 200}
    new_it = forever(lambda: (b for b in ds.batches(B, seed=3) if b["units"].shape[0] == B))
    res["gather"] = time_producer(new_it)
    # the kernel alone, and a copy of the same bytes
    perm = torch.randperm(len(ds), device=dev).to(torch.int32)
    out = ds.ctx.dataset_gather(ds.view, B, Fr, perm=perm, seed=1, crop_frames=Fr, waveform_sec=SEC)
    k = per_launch_us(lambda: ds.ctx.dataset_gather(ds.view, B, Fr, perm=perm, seed=1, crop_frames=Fr, waveform_sec=SEC, out=out))
    moved = 8 * B * Fr * (HOP + C + 2)                  # every output cell is read once (fp32) and written once
    src, dst = torch.empty(moved // 8, device=dev), torch.empty(moved // 8, device=dev)
    c = per_launch_us(lambda: dst.copy_(src))
    res["kernel"] = {**k, "bytes_moved": moved, "GBps": moved / k["median_us"] / 1e3}
    res["copy_same_bytes"] = {**c, "GBps": moved / c["median_us"] / 1e3}
    res["kernel"]["fraction_of_copy_rate"] = res["kernel"]["GBps"] / res["copy_same_bytes"]["GBps"]

    model, _ = synthetic.build_model("CombSub", seed=1, device=dev)
    model.train()
    opt = training.AdamW(model.parameters(), lr=5e-4, weight_decay=0.0)
    bucket = training.GradBucket(model.parameters(), model)
    crit = RSSLoss(256, 2048, 4, device=dev)
    res["gather"]["train_step"] = time_train(new_it, model, opt, crit, bucket)
    if args.baseline:
        base = BaselineLoader(recs, dev)
        base_it = forever(lambda: (b for b in base.batches(B) if b["units"].shape[0] == B))
        res["baseline"] = time_producer(base_it)
        res["baseline"]["train_step"] = time_train(base_it, model, opt, crit, bucket)
        # alternate once more: the spread of the same measurement in one session
        res["gather_again"] = time_producer(new_it)
        res["baseline_again"] = time_producer(base_it)
        res["host_time_ratio_baseline_over_gather"] = res["baseline"]["host_us_per_batch"] / res["gather"]["host_us_per_batch"]
    ds.ctx.poll_error()
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
