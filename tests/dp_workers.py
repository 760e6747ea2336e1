"""What the data-parallel tests share (not a test module): the rank processes of tests/test_dp_host.py (gloo on the CPU, the
oracle stand-ins) and of tests/test_gpu_dp_training.py (gloo, both ranks on device 0), and the helper that runs them.

`run_ranks` starts one process per rank with the `spawn` context, waits for each result and each exit under a time limit of
its own, and fails on a child that does not exit with 0.  Nothing is retried."""
import os
import socket
import types

import numpy as np
import torch
import torch.multiprocessing as mp

HOP = 512
RECT_SCALES = [300, 777, 1531, 2047]          # pinned, below the 4096 samples of 8 frames
NOISE_SEED = 20240611                         # validation's in-kernel noise in the loop test, on both sides
RAGGED_COUNTS = [8, 5, 3, 2]                  # frames per row: ranks 0 / 1 get rows {0, 3} / {1, 2}, padded to 8 / 5 frames


def _paths():
    import sys
    from conftest import PKG, ROOT
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(target, world, args=(), timeout=120):
    """-> [result of rank 0, result of rank 1, ...]: `target(rank, world, port, *args, q)` puts (rank, result) into q."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, *args, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = dict(q.get(timeout=timeout) for _ in range(world))
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0, f"a rank exited with {p.exitcode}"
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return [got[r] for r in range(world)]


def _init(rank, world, port):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def _done(dist):
    dist.barrier()
    dist.destroy_process_group()


# ---- the loss with global denominators, from its definition (the stand-in of the host test) -------------------------------
def share_loss(x_pred, x_true, n_samples, global_n_samples, n_ffts, alpha=1.0, eps=1e-7):
    """tests/ragged_defs.py `ragged_rss_loss` (hop = n_fft) with both denominators taken over `global_n_samples`: the sums
    over the local rows, the number of rows with a frame and of cells that exist over the global ones."""
    total = 0.0
    for N in n_ffts:
        w = torch.hann_window(N, periodic=True, dtype=x_pred.dtype)
        norm = w.pow(2).sum().sqrt()
        rows = sum(1 for n in global_n_samples if n >= N)
        cells = sum(((n - N) // N + 1) * (N // 2 + 1) for n in global_n_samples if n >= N)
        assert rows > 0
        conv, l1 = 0.0, 0.0
        for b, n in enumerate(n_samples):
            if n < N:
                continue
            end = ((n - N) // N) * N + N
            S = [torch.stft(x[b, :end], N, N, N, window=w, center=False, return_complex=True).abs() / norm + eps
                 for x in (x_true, x_pred)]
            conv = conv + torch.linalg.norm(S[0] - S[1]) / torch.linalg.norm(S[0] + S[1])
            l1 = l1 + (S[0].log() - S[1].log()).abs().sum()
        total = total + conv / rows + alpha * l1 / cells
    return total / len(n_ffts)


class OracleLoss:
    """`RSSLoss`'s call signature over `share_loss`."""

    def __init__(self):
        self.scales = None

    def set_scales(self, s):
        self.scales = [int(v) for v in s]

    def __call__(self, x_pred, x_true, n_samples=None, global_n_samples=None):
        return share_loss(x_pred, x_true, n_samples, n_samples if global_n_samples is None else global_n_samples, self.scales)


class OracleSynth(torch.nn.Module):
    """CPU stand-in with the product model's forward signature, `n_frames=` included: the oracle's CombSubFast on every row
    alone at its own length, padded with zeros (what the ragged forward computes)."""

    def __init__(self, sd, cfg):
        super().__init__()
        self.cfg = cfg
        self.buffers_sd = {k: v for k, v in sd.items() if not v.is_floating_point() or "projection_matrix" in k or k == "window"}
        self.p = torch.nn.ParameterDict({k.replace(".", "|"): torch.nn.Parameter(v.clone()) for k, v in sd.items()
                                         if k not in self.buffers_sd})

    def forward(self, units, f0, volume, spk_id, infer=True, noise=None, n_frames=None):
        from oracle import synth as OS
        sd = dict(self.buffers_sd)
        sd.update({k.replace("|", "."): v for k, v in self.p.items()})
        rows = []
        for b, n in enumerate(n_frames):
            sig = OS.combsubfast_forward(sd, self.cfg, units[b:b + 1, :n], f0[b:b + 1, :n], volume[b:b + 1, :n], spk_id[b:b + 1],
                                         infer=infer, noise=noise[b:b + 1, :n * HOP])[0]
            rows.append(torch.nn.functional.pad(sig[0], (0, (units.shape[1] - n) * HOP)))
        return torch.stack(rows), None, None


def ragged_shard(full, counts, rank, world):
    """`rank`'s rows of the global ragged batch `full` (padded to max(counts) frames), cut to the rank's own longest row, with
    `n_frames` and `global_n_frames`: what `AudioDataset.whole_shard` hands `train_step`."""
    _paths()
    from data_loaders import shard_whole
    rows = shard_whole(counts, rank, world)
    n = [counts[j] for j in rows]
    Fr = max(n)
    batch = {k: v[rows] for k, v in full.items()}
    for k in ("units", "f0", "volume"):
        batch[k] = batch[k][:, :Fr].contiguous()
    for k in ("noise", "audio"):
        batch[k] = batch[k][:, :Fr * HOP].contiguous()
    batch["n_frames"], batch["global_n_frames"] = n, list(counts)
    return batch


def host_train_worker(rank, world, port, counts, q):
    """One `training.train_step` on `rank`'s shard of the ragged global batch, on the CPU."""
    _paths()
    import synthetic
    import training
    dist = _init(rank, world, port) if world > 1 else None
    torch.set_num_threads(2)
    model, cfg = synthetic.build_model("CombSubFast", seed=19)
    net = OracleSynth(model.state_dict(), cfg)
    full = synthetic.make_inputs(41, len(counts), max(counts))
    full["audio"] = 0.1 * torch.randn(len(counts), max(counts) * HOP, generator=torch.Generator().manual_seed(3))
    batch = ragged_shard(full, counts, rank, world)
    opt = torch.optim.AdamW(net.parameters(), lr=5e-4, weight_decay=0.0)
    bucket = training.GradBucket(net.parameters())
    loss = training.train_step(net, opt, OracleLoss(), batch, world=world, scales=[300, 777, 1531, 2047], bucket=bucket)
    total = float(training.global_loss(loss, world))
    q.put((rank, (float(loss), total, bucket.flat.numpy().copy(), batch["n_frames"], batch["global_n_frames"])))
    if dist is not None:
        _done(dist)


# ---- the device ----------------------------------------------------------------------------------------------------------
def step_inputs(mode):
    """The global batch of the two-rank step tests: B = 4, 8 frames, injected noise, a random target."""
    _paths()
    import synthetic
    full = synthetic.make_inputs(4300, 4, 8)
    full["audio"] = 0.1 * torch.randn(4, 8 * HOP, generator=torch.Generator().manual_seed(7))
    return full


def device_step(rank, world, mode, dev):
    """One `training.train_step` of CombSub (block 512) on `rank`'s part of the global batch -> (loss, bucket, parameters),
    the last two as flat device tensors.  mode: 'rect' (equal shards of the rectangular batch) or 'ragged' (RAGGED_COUNTS)."""
    _paths()
    import sharding
    import synthetic
    import training
    from ddsp.loss import RSSLoss
    model, _ = synthetic.build_model("CombSub", seed=13)
    model = model.to(dev).train()
    full = step_inputs(mode)
    if mode == "rect":
        batch = sharding.shard_batch(full, world, rank)
    else:
        batch = ragged_shard(full, RAGGED_COUNTS, rank, world)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    opt = training.AdamW(model.parameters(), lr=5e-4, weight_decay=0.0)
    bucket = training.GradBucket(model.parameters(), model)
    loss = training.train_step(model, opt, RSSLoss(256, 2048, 4, device=dev), batch, world=world, scales=RECT_SCALES, bucket=bucket)
    params = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    return loss, bucket.flat, params


def device_step_worker(rank, world, port, mode, q):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    dist = _init(rank, world, port)
    loss, flat, params = device_step(rank, world, mode, dev)
    both = torch.empty(world * flat.numel(), device=dev)
    dist.all_gather_into_tensor(both, flat.contiguous())              # gathered: rank 0 compares the ranks' buckets
    both_p = torch.empty(world * params.numel(), device=dev)
    dist.all_gather_into_tensor(both_p, params)
    res = {"loss": float(loss)}
    if rank == 0:
        b, p = both.view(world, -1), both_p.view(world, -1)
        res.update(buckets_equal=bool(torch.equal(b[0], b[1])), params_equal=bool(torch.equal(p[0], p[1])),
                   bucket=b[0].cpu().numpy().copy())
    q.put((rank, res))
    _done(dist)


def loop_case(root, dev):
    """The synthetic tree of tests/test_gpu_trainer.py (5 short utterances of 3 speakers, tests/golden/ref_solver.npz) as a
    whole-audio dataset, its config and one rectangular training batch of B = 4 with injected noise."""
    _paths()
    import solver_cases as SC
    import synthetic
    from data_loaders import AudioDataset
    from logger.utils import DotDict
    z = SC.load()
    np.save(os.path.join(root, "f0_stats"), SC.f0_stats(z))
    dataset = AudioDataset(None, waveform_sec=0.5, hop_size=SC.HOP, sample_rate=SC.SR, whole_audio=True, n_spk=SC.N_SPK,
                           device=dev, records=SC.records(z))
    scales = [int(s) for s in z["scales"]]
    args = DotDict({"device": "cuda", "env": {"expdir": None, "gpu_id": 0},
                    "data": {"train_path": str(root), "sampling_rate": SC.SR, "block_size": SC.HOP, "encoder_out_channels": SC.N_UNIT},
                    "model": {"type": "CombSub", "n_spk": SC.N_SPK, "n_mag_allpass": 256, "n_mag_harmonic": 512, "n_mag_noise": 256},
                    "loss": {"fft_min": SC.FFT_MIN, "fft_max": SC.FFT_MAX, "n_scale": SC.N_SCALE, "val_scales": scales},
                    "train": {"epochs": 4, "interval_log": 2, "interval_val": 2, "val_batch_frames": 40, "seed": 5}})
    batch = {k: v.to(dev) for k, v in synthetic.make_inputs(4200, 4, 24, n_spk=SC.N_SPK).items()}
    batch["audio"] = (0.1 * torch.randn(4, 24 * SC.HOP, generator=torch.Generator().manual_seed(8))).to(dev)
    return types.SimpleNamespace(SC=SC, dataset=dataset, args=args, batch=batch, scales=scales)


def loop_model(SC, dev):
    from ddsp.vocoder import CombSub
    torch.manual_seed(31)
    return CombSub(SC.SR, SC.HOP, 256, 512, 256, SC.N_UNIT, SC.N_SPK).to(dev)


def loop_worker(rank, world, port, root, q):
    """`solver.train` for 4 steps with a validation every 2, each rank with an experiment directory of its own name."""
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    dist = _init(rank, world, port)
    case = loop_case(root, dev)
    import hipddsp
    import sharding
    import solver
    import training
    from logger.saver import Saver
    hipddsp.seed_from_torch = lambda: NOISE_SEED                         # (the training batch injects its noise)
    from logger.utils import DotDict
    args = DotDict(dict(case.args, env={"expdir": os.path.join(root, f"exp_rank{rank}"), "gpu_id": 0}))
    torch.manual_seed(100 + rank)                                       # ranks start DIFFERENT: the broadcast makes them equal
    model = loop_model(case.SC, dev)
    if rank != 0:
        with torch.no_grad():
            for p in model.parameters():
                p.mul_(1.01)
    opt = training.AdamW(model.parameters(), lr=3e-4, weight_decay=0.0)
    training.broadcast_state(model, opt)
    logged = []
    log_value = Saver.log_value
    Saver.log_value = lambda self, d: (logged.append((self.global_step, dict(d))), log_value(self, d))[1]
    crit = training_loss(case, dev)
    mine = sharding.shard_batch(case.batch, world, rank)
    solver.train(args, 0, model, opt, crit, [mine], types.SimpleNamespace(dataset=case.dataset), max_steps=4)
    checksum = float(sum(p.detach().double().sum() for p in model.parameters()))
    q.put((rank, {"logged": logged, "checksum": checksum, "val_scales_used": crit.last_scales}))
    _done(dist)


def training_loss(case, dev):
    from ddsp.loss import RSSLoss
    SC = case.SC
    return RSSLoss(SC.FFT_MIN, SC.FFT_MAX, SC.N_SCALE, device=dev)
