"""The reference's `solver.py` (`test`, `train`) on the device path.

Training is `training.train_step` over the loader's epochs with a `GradBucket`; the loss value is read back only when it is
logged, so a step that does not log does not synchronise.

Validation (`validate`, which `test` calls) differs from the reference's loop in HOW it runs, not in what it reports.  The
reference renders every file twice at B = 1 (reconstruction, and conversion to the next speaker), scores it and reads the loss
back - two dependent launch chains and a host synchronisation per file (`solver.py:29-74`).  Here the files go through
`AudioDataset.whole_batches` as ragged groups; per group the conversion leg's f0 and target ids come from one kernel
(`ddsp_vc_f0_map`, no host round trip), ONE ragged forward of 2 B rows renders both legs, and `RSSLoss.rows` scores the B
reconstruction rows, one loss per utterance.  The losses stay on the device until every group is done; one read-back follows,
and their mean - every file counts once, the reference's `test_loss` - is returned.

One divergence: the reference draws the loss's scales per FILE; here a draw serves a GROUP (all its rows are scored in one
call), or, with `scales=`, one pinned draw serves the whole pass.  Pinning is the recommended use: the validation losses of
different steps are then measured with the same yardstick and become comparable (`args.loss.val_scales` in the config).

Data parallel (`ranks=`, default `training.Ranks.current()`: the process group `train.py` initialised, or one process).  A
training step all-reduces the summed gradient bucket and nothing else; the loss's scales and the noise seed of a step are pure
functions of (`train.seed`, step[, rank]).  The global loss is formed (`training.global_loss`, one scalar all_reduce) on the
steps that log, so a step that does not log synchronises with the host on no rank.  Validation deals the global groups to the
ranks round robin, every rank scores its groups, the per-file losses are gathered once per pass and every rank returns the same
mean over the files; the scales must be pinned (a draw would differ per group).  Rank 0 alone logs and writes checkpoints - the
others wait at a barrier - and its "best" decision is broadcast so that every rank takes the same branch."""
import time

import numpy as np
import torch

import hipddsp
from logger.saver import Saver
from training import GradBucket, Ranks, global_loss, step_noise_seed, step_scales, train_step

VAL_BATCH_FRAMES = 8192     # padded frames of a validation group when nothing else is asked for (the forward sees twice that)


def target_speaker(src_spk_id, n_spk):
    """The speaker validation converts `src_spk_id` to (`solver.py:46-48`): (src + 1) % n_spk, and 0 becomes 1.  The host
    form of what `ddsp_vc_f0_map` computes per row."""
    tgt = (int(src_spk_id) + 1) % int(n_spk)
    return 1 if tgt == 0 else tgt


def lfo_table(lfo_stats, n_spk):
    """`f0_stats.npy`'s dict {str(speaker id): mean log f0} -> float32 (n_spk,), entry id - 1; NaN where a speaker has none."""
    table = np.full(int(n_spk), np.nan, dtype=np.float32)
    for k, v in lfo_stats.items():
        if 1 <= int(k) <= int(n_spk):
            table[int(k) - 1] = v
    return table


def check_validation_files(names, frames, hop, fft_max, spk_ids=None, table=None):
    """Host checks of a validation pass, before anything is launched: every utterance holds `fft_max` samples (so it has a
    frame at any scale the loss can draw), and its speaker and the speaker it is converted to have a log-f0 statistic.
    ValueError names the file."""
    for i, (name, n) in enumerate(zip(names, frames)):
        if int(n) * int(hop) < int(fft_max):
            raise ValueError(f"{name}: the validation utterance holds {int(n) * int(hop)} samples, fewer than fft_max = "
                             f"{int(fft_max)}: it has no frame at the loss's largest scales")
        if table is not None:
            for spk in (spk_ids[i], target_speaker(spk_ids[i], len(table))):
                if not 1 <= spk <= len(table) or np.isnan(table[spk - 1]):
                    raise ValueError(f"{name}: speaker {spk} has no entry in f0_stats.npy (preprocess(..., gen_stats=True) "
                                     "writes it from the training set)")


def validate(args, model, loss_func, dataset, saver=None, batch_frames=None, scales=None, noise=None, details=None, ranks=None):
    """The reference's `test` over `dataset` (a whole-audio `AudioDataset`) -> the mean of the per-file losses (module
    docstring).  batch_frames: a group's padded size in frames (default VAL_BATCH_FRAMES).  scales: one pinned draw of the
    loss's scales for the whole pass (default None: a fresh draw per group; the reference draws per file).  noise: {file
    name: U[0,1) draws (n_frames * block_size,)} in place of the in-kernel noise, for both legs (the parity form, like
    `noise=` on the synthesisers).  details: a dict that receives `names`, `losses` (float64 numpy, per file in that order),
    `rtf`.  With a `saver`, the ground truth, the reconstruction and the conversion of every file are logged under the
    reference's tags.  RTF is the wall time of the whole pass (gather, both legs, loss; one synchronisation at its end) over
    the duration of the audio.  ranks: module docstring; `details` then holds every rank's files, in gathered order."""
    ranks = Ranks.current() if ranks is None else ranks
    if ranks.world > 1 and scales is None:
        raise ValueError("validate: data-parallel validation needs pinned scales (loss.val_scales): a draw would differ per group")
    hop = dataset.hop_size
    check_validation_files(dataset.paths, dataset.whole, hop, loss_func.fft_max)
    lfo_stats = np.load(f"{args.data.train_path}/f0_stats.npy", allow_pickle=True).item()
    table = lfo_table(lfo_stats, args.model.n_spk)
    check_validation_files(dataset.paths, dataset.whole, hop, loss_func.fft_max, dataset.spk_ids, table)
    if ranks.rank == 0:
        print(f" [*] validating {len(dataset.paths)} files...")
    model.eval()
    ctx = hipddsp.context_for(dataset.device)
    lfo = torch.from_numpy(table).to(dataset.device)
    spk_of = dict(zip(dataset.paths, dataset.spk_ids))
    names, losses, frames = [], [], 0
    st_time = time.time()
    with torch.no_grad():
        groups = dataset.whole_groups(VAL_BATCH_FRAMES if batch_frames is None else batch_frames)
        for batch in (dataset.whole_batch(g) for g in groups[ranks.rank::ranks.world]):
            n, group = batch["n_frames"], batch["name"]
            B = len(n)
            f0_vc, tgt = ctx.vc_f0_map(batch["f0"], batch["spk_id"], lfo, ctx.ragged_counts(n))
            extra = {}
            if noise is not None:
                draw = torch.full((B, batch["audio"].shape[1]), 0.5, device=dataset.device)
                for b, fn in enumerate(group):
                    draw[b, :n[b] * hop] = noise[fn].to(dataset.device)
                extra["noise"] = torch.cat([draw, draw])
            signal, _, _ = model(torch.cat([batch["units"], batch["units"]]), torch.cat([batch["f0"], f0_vc]),
                                 torch.cat([batch["volume"], batch["volume"]]), torch.cat([batch["spk_id"], tgt]),
                                 n_frames=n + n, **extra)
            if scales is not None:
                loss_func.set_scales(scales)
            losses.append(loss_func.rows(signal[:B], batch["audio"], [k * hop for k in n]))
            names += group
            frames += sum(n)
            if saver is not None:
                for b, fn in enumerate(group):
                    src = spk_of[fn]
                    end = n[b] * hop
                    saver.log_audio({fn + "/gt.wav": batch["audio"][b:b + 1, :end], fn + "/pred.wav": signal[b:b + 1, :end],
                                     f"{fn}/vc_{src}_to_{target_speaker(src, args.model.n_spk)}.wav": signal[B + b:B + b + 1, :end]})
        if ranks.world > 1:
            names, losses, frames = _gather_files(losses, groups, dataset, ranks)
        per_file = torch.cat(losses).cpu()              # the pass's one read-back: it waits for every group
    run_time = time.time() - st_time
    ctx.poll_error()
    per_file = per_file.double().numpy()
    test_loss = float(per_file.mean())
    rtf = run_time / (frames * hop / args.data.sampling_rate)
    if details is not None:
        details.update(names=names, losses=per_file, rtf=rtf)
    if ranks.rank == 0:
        print(f" [*] validation loss {test_loss} | RTF {rtf} ({run_time} s for {frames * hop / args.data.sampling_rate} s of audio)")
    return test_loss


def _gather_files(losses, groups, dataset, ranks):
    """The pass's one exchange: every rank's per-file losses in a slot of len(dataset) floats (all_gather), cut by the file
    counts the round-robin deal gives each rank - a pure function of the lengths, so nothing but the losses travels."""
    import torch.distributed as dist
    mine = torch.cat(losses) if losses else torch.zeros(0, device=dataset.device)
    slot = torch.zeros(len(dataset.paths), device=dataset.device)
    slot[:mine.numel()] = mine
    out = torch.empty(ranks.world * slot.numel(), device=dataset.device)
    dist.all_gather_into_tensor(out, slot)
    all_names, all_losses = [], []
    for r in range(ranks.world):
        files = [i for g in groups[r::ranks.world] for i in g]
        all_names += [dataset.paths[i] for i in files]
        all_losses.append(out[r * slot.numel():r * slot.numel() + len(files)])
    return all_names, all_losses, sum(dataset.whole)


def test(args, model, loss_func, loader_test, saver, ranks=None):
    """The reference's signature: `loader_test` is `get_data_loaders`' validation loader (its `.dataset` is walked in ragged
    groups).  `args.train.val_batch_frames` and `args.loss.val_scales` (both optional in the YAML) set the group size and
    pin the scales."""
    return validate(args, model, loss_func, loader_test.dataset, saver, batch_frames=args.train.val_batch_frames,
                    scales=args.loss.val_scales, ranks=ranks)


def train(args, initial_global_step, model, optimizer, loss_func, loader_train, loader_test, max_steps=None, scales=None,
          ranks=None):
    """The reference's loop (`solver.py:85-143`): a step per batch of `loader_train` for `args.train.epochs` epochs, a log line
    every `interval_log` steps, and every `interval_val` steps a validation, the checkpoint of that step and, if the validation
    loss improved, `model_best.pt`.  max_steps: return after that many steps of this call.  scales: pin the training loss's
    draw (tests; default: drawn per step as the reference does - under data parallelism by `training.step_scales`).
    ranks: module docstring."""
    ranks = Ranks.current() if ranks is None else ranks
    world = ranks.world
    if world > 1 and not args.loss.val_scales:
        raise ValueError("train: data-parallel training needs loss.val_scales (validation's pinned scales) in the config")
    seed = int(args.train.seed or 0)
    saver = Saver(args, initial_global_step=initial_global_step, rank=ranks.rank)
    bucket = GradBucket(model.parameters(), model)
    best_loss = np.inf
    num_batches = len(loader_train)
    model.train()
    done = 0
    saver.log_info(f"training from step {initial_global_step}" + (f" on {world} ranks" if world > 1 else ""))
    for epoch in range(args.train.epochs):
        for batch_idx, data in enumerate(loader_train):
            saver.global_step_increment()
            step_scale = scales
            if world > 1:
                if "noise" not in data:
                    data["noise_seed"] = step_noise_seed(seed, saver.global_step, ranks.rank)
                if scales is None:
                    step_scale = step_scales(seed, saver.global_step, loss_func.fft_min, loss_func.fft_max, loss_func.n_scale)
            loss = train_step(model, optimizer, loss_func, data, world=world, scales=step_scale, bucket=bucket)
            if saver.global_step % args.train.interval_log == 0:
                # the only read-back of a training step, and only when it is logged (with it, the one scalar all_reduce)
                value = global_loss(loss, world, shares="global_n_frames" in data).item()
                saver.log_info(f"step {saver.global_step} | epoch {epoch} batch {batch_idx}/{num_batches} | {args.env.expdir} | "
                               f"{args.train.interval_log / saver.get_interval_time():.2f} batch/s | loss {value:.3f} | "
                               f"{saver.get_total_time()}")
                saver.log_value({"train/loss": value})
            if saver.global_step % args.train.interval_val == 0:
                test_loss = test(args, model, loss_func, loader_test, saver if ranks.rank == 0 else None, ranks=ranks)
                saver.log_info(f"step {saver.global_step} | validation loss {test_loss:.3f}")
                saver.log_value({"validation/loss": test_loss})
                saver.save_model(model, optimizer, postfix=f"{saver.global_step}")
                if _rank0_decides(test_loss < best_loss, ranks):
                    saver.log_info(f"step {saver.global_step} | best validation loss so far: model_best.pt updated")
                    saver.save_model(model, optimizer, postfix="best")
                    best_loss = test_loss
                if world > 1:
                    import torch.distributed as dist
                    dist.barrier()                      # the others wait here while rank 0 writes
                model.train()
            done += 1
            if max_steps is not None and done >= max_steps:
                return


def _rank0_decides(flag, ranks):
    """`flag` as rank 0 sees it, on every rank (one broadcast of a byte; one process: `flag`)."""
    if ranks.world == 1:
        return bool(flag)
    import torch.distributed as dist
    box = [bool(flag)]
    dist.broadcast_object_list(box, src=0)
    return box[0]
