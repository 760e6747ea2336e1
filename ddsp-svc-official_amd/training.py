"""Training-side glue of the reference (`train.py:41-48`, `solver.py:100-114`) on the device path: an AdamW whose
update runs as a libddsp_amd kernel (state dict compatible with `torch.optim.AdamW`, so `Saver` checkpoints resume),
the data-parallel gradient exchange, and one training step."""
import torch

import hipddsp


class AdamW(torch.optim.Optimizer):
    """Same constructor / defaults / state keys ('step', 'exp_avg', 'exp_avg_sq') as torch.optim.AdamW (no amsgrad)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        """grad_scale: every gradient is multiplied by it as the kernel reads it (the 1 / world of a data-parallel mean over a
        bucket that holds the sum); the gradients themselves are not written.  1.0 is the call without it, bit for bit."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            # parameters that can share one library call: same device, same step count, contiguous storage
            batches = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError("AdamW kernel runs on a HIP device only (no CPU fallback)")
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["step"] += 1
                if not p.data.is_contiguous():
                    raise ValueError("AdamW kernel needs contiguous parameters")
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                batches.setdefault((p.device, int(st["step"])), []).append((p, g, st["exp_avg"], st["exp_avg_sq"]))
            for (device, step), items in batches.items():
                ps, gs, ms, vs = zip(*items)
                hipddsp.context_for(device).adamw_step_multi(ps, gs, ms, vs, group["lr"], b1, b2, group["eps"],
                                                             group["weight_decay"], step, grad_scale=grad_scale)
                # the kernel writes through the pointers: count the write as torch.optim.AdamW's in-place updates do, so that
                # the models' prepared weights (hipddsp.WeightTable) follow the step
                torch.autograd.graph.increment_version(ps)
        return loss


def allreduce_gradients(params, world, group=None):
    """Data-parallel mean of the gradients: one flat 14 MB bucket, one RCCL all_reduce.  The backward of
    the control network is a single library call, so there is nothing to overlap the exchange with except the next
    step's host work; at 7 x 153 GB/s of xGMI the bucket takes tens of microseconds."""
    if world <= 1:
        return
    import torch.distributed as dist
    grads = [p.grad for p in params if p.grad is not None]
    flat = torch.cat([g.reshape(-1) for g in grads])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    flat /= world
    off = 0
    for g in grads:
        n = g.numel()
        g.copy_(flat[off:off + n].view_as(g))
        off += n


class GradBucket:
    """All gradients of a model in ONE flat fp32 buffer: every `p.grad` is a view into it, so the data-parallel exchange
    is a single collective on memory that already holds the gradients (no `cat` before, no `copy_` after - 14 MB each
    way per step otherwise).  autograd accumulates into an existing `.grad` in place, so the views survive a backward
    pass; `zero()` replaces `optimizer.zero_grad()` (whose default, set_to_none, would drop the views)."""

    def __init__(self, params, model=None):
        """`model`: the synthesiser whose parameters these are - its control network then receives its gradients directly
        in the bucket (`Unit2Control._grads_in_place`, a one-shot token that `zero()` arms) instead of through autograd's
        accumulation."""
        self.params = [p for p in params if p.requires_grad]
        n = sum(p.numel() for p in self.params)
        ref = self.params[0]
        self.flat = torch.zeros(n, device=ref.device, dtype=torch.float32)
        off = 0
        for p in self.params:
            p.grad = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        self._net = model.unit2ctrl if model is not None and hasattr(model, "unit2ctrl") else None

    def zero(self):
        """Zero every gradient and ARM the control network's direct write for the NEXT backward pass only: the library
        overwrites (`=`) the bucket's views instead of handing gradients to autograd, which is right exactly once per
        zeroed bucket.  A second backward before the next `zero()` (micro-batches, two losses) finds the token spent and
        goes through autograd's accumulation again (`Unit2Control.backward_flat`)."""
        self.flat.zero_()
        if self._net is not None:
            self._net._grads_in_place = True

    def allreduce(self, world, group=None, average=True):
        """One all_reduce over the ranks (RCCL over xGMI on GPUs): the mean, or with `average=False` the SUM.  A data-parallel
        `train_step` with `training.AdamW` leaves the sum here - the bucket then holds the sum, not the mean, after the step:
        the 1 / world is applied by the optimizer's kernel as it reads the gradients (`AdamW.step(grad_scale=)`), or is not
        wanted at all (loss shares of a ragged global batch, whose gradients add up to the global gradient)."""
        if world <= 1:
            return
        import torch.distributed as dist
        dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)
        if average:
            self.flat /= world


class Ranks:
    """The data-parallel job this process is a rank of: `rank` of `world`.  `Ranks.current()` reads it from
    `torch.distributed` when a process group is initialised (`train.py` does that when it is started under
    `torch.distributed.run`) and is one process otherwise."""

    def __init__(self, rank=0, world=1):
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"Ranks: rank {rank} of {world}")
        self.rank, self.world = int(rank), int(world)

    @classmethod
    def current(cls):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return cls(dist.get_rank(), dist.get_world_size())
        return cls()


def _mix(*words):
    """A 63-bit hash of a few ints (splitmix64 steps), the same on every host."""
    h = 0x9E3779B97F4A7C15
    for w in words:
        h = (h ^ (int(w) & 0xFFFFFFFFFFFFFFFF)) * 0xBF58476D1CE4E5B9 & 0xFFFFFFFFFFFFFFFF
        h = (h ^ (h >> 27)) * 0x94D049BB133111EB & 0xFFFFFFFFFFFFFFFF
        h ^= h >> 31
    return h & ((1 << 63) - 1)


def step_scales(seed, step, fft_min, fft_max, n_scale):
    """The loss's scales of training step `step` under data parallelism: `torch.randint(fft_min, fft_max, (n_scale,))` from a
    generator seeded with (seed, step) - a pure function of its arguments, so every rank and a resumed run agree on the draw
    without communication."""
    g = torch.Generator()
    g.manual_seed(_mix(seed, step, 1))
    return [int(v) for v in torch.randint(int(fft_min), int(fft_max), (int(n_scale),), generator=g)]


def step_noise_seed(seed, step, rank):
    """The seed of the in-kernel noise of training step `step` on `rank`: ranks draw different noise, a resumed run the same."""
    return _mix(seed, step, 2, rank) & ((1 << 62) - 1)


def broadcast_state(model, optimizer, src=0):
    """Replicas start equal: `src`'s parameters and buffers, and the optimizer state that exists there (after a resume; every
    rank has loaded the same file, so the key sets agree), are broadcast in place."""
    import torch.distributed as dist
    with torch.no_grad():
        for t in list(model.parameters()) + list(model.buffers()):
            dist.broadcast(t.data, src)
        for group in optimizer.param_groups:
            for p in group["params"]:
                for k in ("exp_avg", "exp_avg_sq"):
                    if k in optimizer.state.get(p, {}):
                        dist.broadcast(optimizer.state[p][k], src)
    torch.autograd.graph.increment_version(list(model.parameters()))


def global_loss(loss, world, group=None, shares=True):
    """The loss of the global batch from this rank's `train_step` value, as a device scalar: the SUM of the ranks' values when
    they are shares (a ragged step with `global_n_frames`), their MEAN with `shares=False` (a rectangular step with equal
    shards).  One all_reduce of a scalar, in which every rank takes part - call it on the steps that log only."""
    if world <= 1:
        return loss
    import torch.distributed as dist
    total = loss.detach().clone()
    dist.all_reduce(total, op=dist.ReduceOp.SUM, group=group)
    return total if shares else total / world


def train_step(model, optimizer, loss_fn, batch, world=1, scales=None, bucket=None):
    """One step of `solver.train` (`solver.py:110-114`): zero_grad -> forward(infer=False) -> loss -> backward -> step.
    `scales` pins the loss's n_fft draw (ranks of a data-parallel job must share it; both terms of the loss
    are batch means, `ddsp/loss.py:20-22`, so with equal shards the mean of the rank losses is the global loss and the
    mean of the rank gradients its gradient).  `bucket`: a GradBucket over the model's parameters (one flat collective); with
    `training.AdamW` and `world > 1` it is left holding the SUM of the rank gradients and the optimizer's kernel applies the
    1 / world (another optimizer gets the mean in the bucket, as before).
    `batch["n_frames"]` (B ints, optional): a ragged batch of whole utterances - the counts go to the model, and times the
    block size to the loss, whose terms are then means over the rows' own frames.  Ranks with unequal shards hold unequal
    `batch["noise_seed"]` (optional): the seed of the in-kernel noise (default: drawn from torch's generator).
    numbers of loss cells, so the mean of the rank losses is not the global loss: `world > 1` with `n_frames` raises
    ValueError (such a batch trains on one process) UNLESS the batch also carries `batch["global_n_frames"]`, the frame counts
    of all ranks' rows (the same list on every rank, this rank's rows among them).  The loss then takes its denominators from
    the global counts (`RSSLoss.forward(..., global_n_samples=)`): the returned value is this rank's SHARE of the global loss
    (`global_loss` adds the shares up), the gradients are summed over the ranks and the optimizer steps on the sum."""
    n_frames = batch.get("n_frames")
    global_n_frames = batch.get("global_n_frames")
    ragged = {}
    if n_frames is not None:
        if world != 1 and global_n_frames is None:
            raise ValueError("train_step: a ragged batch (n_frames) trains on one process - the mean of the rank losses of "
                             "unequal shards is not the global loss - unless it carries global_n_frames, the counts of all "
                             "ranks' rows")
        n_frames = hipddsp.check_n_frames(n_frames, batch["units"].shape[0], batch["units"].shape[1])
        ragged = {"n_frames": n_frames}
    elif global_n_frames is not None:
        raise ValueError("train_step: global_n_frames comes with n_frames, the counts of this rank's rows")
    if bucket is not None:
        bucket.zero()
    else:
        optimizer.zero_grad()
    signal, _, _ = model(batch["units"].float(), batch["f0"], batch["volume"], batch["spk_id"], infer=False,
                         **({"noise": batch["noise"]} if "noise" in batch else {}),
                         **({"noise_seed": batch["noise_seed"]} if "noise_seed" in batch else {}), **ragged)
    if scales is not None:
        loss_fn.set_scales(scales)
    if n_frames is not None:
        hop = signal.shape[1] // batch["units"].shape[1]
        shares = {} if global_n_frames is None else {"global_n_samples": [int(n) * hop for n in global_n_frames]}
        loss = loss_fn(signal, batch["audio"], n_samples=[n * hop for n in n_frames], **shares)
    else:
        loss = loss_fn(signal, batch["audio"])
    loss.backward()
    fused = world > 1 and bucket is not None and isinstance(optimizer, AdamW)
    if bucket is not None:
        bucket.allreduce(world, average=not (fused or global_n_frames is not None))
    elif global_n_frames is not None and world > 1:
        raise ValueError("train_step: loss shares (global_n_frames) are summed over the ranks in a GradBucket")
    else:
        allreduce_gradients(list(model.parameters()), world)
    if fused and global_n_frames is None:
        optimizer.step(grad_scale=1.0 / world)
    else:
        optimizer.step()
    return loss.detach()
