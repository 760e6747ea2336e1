"""Steps per second of `solver.train` under data parallelism.  Run on a node with N GPUs:
    python -m torch.distributed.run --nproc-per-node N tools/dp_train_time.py [--steps 200] [--out profiles/dp_train_time.json]
(one process, N = 1: `python tools/dp_train_time.py`; `--dist-backend gloo` with every rank on one GPU is the rehearsal form,
which measures the control flow and says nothing about RCCL over xGMI).
CombSub at block 512, a global batch of 32 crops of 2 s at 44.1 kHz split over the ranks, a synthetic dataset of 64 files of
3 to 8 s resident on every rank's GPU, the loss's scales from `training.step_scales`, no validation and no logging inside the
timed window (a step that does not log does not synchronise).  Per run: `--warmup` steps, one synchronisation and barrier,
`--steps` steps through `solver.train`, one synchronisation and barrier; the wall time of the slowest rank counts.
`--unfused` also times the same steps with the gradient mean formed in a pass of its own (`GradBucket.allreduce(average=True)`,
then `AdamW.step()`), the form before the scale moved into the optimizer's launch."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ddsp-svc-official_amd"))
import data_loaders as DL  # noqa: E402
import solver  # noqa: E402
import training  # noqa: E402
from ddsp.loss import RSSLoss  # noqa: E402
from ddsp.vocoder import CombSub  # noqa: E402
from logger.utils import DotDict  # noqa: E402

SR, HOP, SEC, C, B, N_SPK = 44100, 512, 2.0, 256, 32, 4


def make_records(n_files, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    recs = []
    for i in range(n_files):
        n = int(rng.integers(3 * SR, 8 * SR))
        fr = n // HOP + 1
        recs.append({"name": f"{1 + i % N_SPK}/f{i:04d}", "audio": (0.1 * rng.standard_normal(n, dtype=np.float32)),
                     "duration": n / SR, "spk_id": 1 + i % N_SPK, "f0": rng.uniform(80, 600, fr).astype(np.float32),
                     "volume": rng.uniform(0, 0.3, fr).astype(np.float32),
                     "units": [rng.standard_normal((fr, C), dtype=np.float32)]})
    return recs


class _Forever:
    """`dataset.batches` epoch after epoch (the timed window never meets the end of the loader)."""

    def __init__(self, dataset, ranks):
        self.dataset, self.ranks = dataset, ranks

    def __len__(self):
        return len(self.dataset) // B

    def __iter__(self):
        return self.dataset.batches(B, 0, self.ranks.rank, self.ranks.world, even=True)


def timed(args, ranks, model, opt, crit, loader, steps, dev):
    import torch.distributed as dist
    torch.cuda.synchronize(dev)
    if ranks.world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    solver.train(args, 0, model, opt, crit, loader, None, max_steps=steps, ranks=ranks)
    torch.cuda.synchronize(dev)
    dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
    if ranks.world > 1:
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    return float(dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--dist-backend", default=None)
    ap.add_argument("--unfused", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dp_train_time.json"))
    cmd = ap.parse_args()
    import train as train_cli
    args = DotDict({"device": "cuda", "env": {"expdir": tempfile.mkdtemp(prefix="dp_train_time_"), "gpu_id": 0},
                    "data": {"sampling_rate": SR, "block_size": HOP},
                    "loss": {"fft_min": 256, "fft_max": 2048, "n_scale": 4, "val_scales": [300, 777, 1200, 2000]},
                    "train": {"epochs": 10 ** 6, "interval_log": 10 ** 9, "interval_val": 10 ** 9, "seed": 0, "batch_size": B,
                              "cache_device": "cuda"}})
    ranks = train_cli.init_ranks(args, cmd.dist_backend)
    dev = torch.device(args.device if ranks.world > 1 else "cuda:0")
    if B % ranks.world:
        raise SystemExit(f"the global batch of {B} does not divide by {ranks.world} ranks")
    torch.manual_seed(1)
    model = CombSub(SR, HOP, 256, 512, 256, C, N_SPK).to(dev)
    opt = training.AdamW(model.parameters(), lr=3e-4, weight_decay=0.0)
    if ranks.world > 1:
        training.broadcast_state(model, opt)
    crit = RSSLoss(256, 2048, 4, device=dev)
    dataset = DL.AudioDataset(None, waveform_sec=SEC, hop_size=HOP, sample_rate=SR, n_spk=N_SPK, device=dev,
                              records=make_records(64))
    loader = _Forever(dataset, ranks)
    out = {"ranks": ranks.world, "backend": cmd.dist_backend or ("nccl" if ranks.world > 1 else None), "global_batch": B,
           "steps": cmd.steps, "warmup": cmd.warmup, "gpu": torch.cuda.get_device_name(dev)}
    legs = [("fused", None)]
    if cmd.unfused and ranks.world > 1:
        legs.append(("unfused", True))
    for tag, unfused in legs:
        plain, step = training.GradBucket.allreduce, training.AdamW.step
        if unfused:          # the mean in a pass of its own over the bucket, and an optimizer step that scales nothing
            training.GradBucket.allreduce = lambda self, world, group=None, average=True: plain(self, world, group, True)
            training.AdamW.step = lambda self, closure=None, grad_scale=1.0: step(self, closure)
        try:
            timed(args, ranks, model, opt, crit, loader, cmd.warmup, dev)
            dt = timed(args, ranks, model, opt, crit, loader, cmd.steps, dev)
        finally:
            training.GradBucket.allreduce, training.AdamW.step = plain, step
        out[tag] = {"seconds": dt, "steps_per_s": cmd.steps / dt, "ms_per_step": 1e3 * dt / cmd.steps,
                    "clips_per_s": B * cmd.steps / dt}
    if ranks.rank == 0:
        print(json.dumps(out), flush=True)
        os.makedirs(os.path.dirname(cmd.out), exist_ok=True)
        with open(cmd.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    if ranks.world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
