"""The reference's `train.py` on the device path: `python train.py -c <config.yaml>` trains the model the config names on the
tree `preprocess.py` wrote, validates every `train.interval_val` steps, writes `model_<step>.pt` / `model_best.pt` into
`env.expdir` and resumes from the freshest of them.  Checkpoints have the reference's key layout ({global_step, model,
optimizer} with `torch.optim.AdamW`'s state keys), so either side loads the other's files.

Data parallel: `python -m torch.distributed.run --nproc-per-node N train.py -c <config.yaml>` trains on N GPUs of one node.
`WORLD_SIZE`, `RANK` and `LOCAL_RANK` (set by the launcher) are read; rank r uses GPU `LOCAL_RANK`, the process group is `nccl`
(or the backend `--dist-backend` names; `gloo` with every rank on one GPU is the rehearsal form), rank 0's parameters and
optimizer state are broadcast before the first step, `train.batch_size` is the global batch, and rank 0 alone writes into
`env.expdir`.  Without `WORLD_SIZE` in the environment nothing of this runs."""
import argparse
import os

import torch

from data_loaders import get_data_loaders
from ddsp.loss import RSSLoss
from ddsp.vocoder import CombSub, CombSubFast, Sins
from logger import utils
from solver import train
from training import AdamW, Ranks, broadcast_state


def build_model(args):
    """The synthesiser `args.model.type` names, constructed from the config as `ddsp.vocoder.load_model` does."""
    common = dict(sampling_rate=args.data.sampling_rate, block_size=args.data.block_size, n_unit=args.data.encoder_out_channels,
                  n_spk=args.model.n_spk, c=args.model.c)
    if args.model.type == "Sins":
        return Sins(n_harmonics=args.model.n_harmonics, n_mag_allpass=args.model.n_mag_allpass,
                    n_mag_noise=args.model.n_mag_noise, **common)
    if args.model.type == "CombSub":
        return CombSub(n_mag_allpass=args.model.n_mag_allpass, n_mag_harmonic=args.model.n_mag_harmonic,
                       n_mag_noise=args.model.n_mag_noise, **common)
    if args.model.type == "CombSubFast":
        return CombSubFast(**common)
    raise ValueError(f" [x] Unknown Model: {args.model.type}")


def init_ranks(args, backend=None):
    """The process group of a run started under `torch.distributed.run` -> `Ranks`; one process (and nothing initialised)
    without `WORLD_SIZE`.  Rank r takes GPU `LOCAL_RANK` (modulo the GPUs there are: ranks may share one under gloo) and
    `args.device` / `args.env.gpu_id` / `args.train.cache_device` are pointed at it."""
    if "WORLD_SIZE" not in os.environ:
        return Ranks()
    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    import torch.distributed as dist
    torch.cuda.set_device(local)
    args["device"] = f"cuda:{local}"                    # (item access: attribute access hands out copies of nested dicts)
    args["env"]["gpu_id"] = local
    args["train"]["cache_device"] = args["device"]
    if backend in (None, "nccl"):
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    return Ranks(rank, world)


def main(config, max_steps=None, dist_backend=None):
    args = utils.load_config(config)
    ranks = init_ranks(args, dist_backend)              # before the model is built
    if ranks.rank == 0:
        print(" > config:", config)
        print(" >    exp:", args.env.expdir)
    if ranks.world == 1 and torch.device(args.device).type == "cuda" and args.env.gpu_id is not None:
        torch.cuda.set_device(args.env.gpu_id)
    # the model lives on the device before the optimizer sees its parameters: a resumed state is then loaded next to them
    model = build_model(args).to(args.device)
    optimizer = AdamW(model.parameters())
    initial_global_step, model, optimizer = utils.load_model(args.env.expdir, model, optimizer, device=args.device)
    for param_group in optimizer.param_groups:          # the YAML decides, also after a resume
        param_group["lr"] = args.train.lr
        param_group["weight_decay"] = args.train.weight_decay
    loss_func = RSSLoss(args.loss.fft_min, args.loss.fft_max, args.loss.n_scale, device=args.device)
    if ranks.world > 1:
        broadcast_state(model, optimizer)               # replicas start equal (a random initialisation; a resume already is)
    loader_train, loader_valid = get_data_loaders(args, whole_audio=False, rank=ranks.rank, world=ranks.world)
    train(args, initial_global_step, model, optimizer, loss_func, loader_train, loader_valid, max_steps=max_steps, ranks=ranks)
    if ranks.world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("-c", "--config", type=str, required=True, help="path to the config file")
    parser.add_argument("--max-steps", type=int, default=None, help="stop after this many steps of this run")
    parser.add_argument("--dist-backend", type=str, default=None,
                        help="torch.distributed backend under torch.distributed.run (default nccl; gloo: the rehearsal form)")
    cmd = parser.parse_args()
    main(cmd.config, cmd.max_steps, cmd.dist_backend)
