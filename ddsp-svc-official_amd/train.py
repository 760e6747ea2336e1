"""The reference's `train.py` on the device path: `python train.py -c <config.yaml>` trains the model the config names on the
tree `preprocess.py` wrote, validates every `train.interval_val` steps, writes `model_<step>.pt` / `model_best.pt` into
`env.expdir` and resumes from the freshest of them.  Checkpoints have the reference's key layout ({global_step, model,
optimizer} with `torch.optim.AdamW`'s state keys), so either side loads the other's files."""
import argparse

import torch

from data_loaders import get_data_loaders
from ddsp.loss import RSSLoss
from ddsp.vocoder import CombSub, CombSubFast, Sins
from logger import utils
from solver import train
from training import AdamW


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


def main(config, max_steps=None):
    args = utils.load_config(config)
    print(" > config:", config)
    print(" >    exp:", args.env.expdir)
    if torch.device(args.device).type == "cuda" and args.env.gpu_id is not None:
        torch.cuda.set_device(args.env.gpu_id)
    # the model lives on the device before the optimizer sees its parameters: a resumed state is then loaded next to them
    model = build_model(args).to(args.device)
    optimizer = AdamW(model.parameters())
    initial_global_step, model, optimizer = utils.load_model(args.env.expdir, model, optimizer, device=args.device)
    for param_group in optimizer.param_groups:          # the YAML decides, also after a resume
        param_group["lr"] = args.train.lr
        param_group["weight_decay"] = args.train.weight_decay
    loss_func = RSSLoss(args.loss.fft_min, args.loss.fft_max, args.loss.n_scale, device=args.device)
    loader_train, loader_valid = get_data_loaders(args, whole_audio=False)
    train(args, initial_global_step, model, optimizer, loss_func, loader_train, loader_valid, max_steps=max_steps)


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("-c", "--config", type=str, required=True, help="path to the config file")
    parser.add_argument("--max-steps", type=int, default=None, help="stop after this many steps of this run")
    cmd = parser.parse_args()
    main(cmd.config, cmd.max_steps)
