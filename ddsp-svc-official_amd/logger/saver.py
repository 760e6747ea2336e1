"""The reference's `logger/saver.py`: the experiment directory of a training run - `config.yaml` (which
`ddsp.vocoder.load_model` reads next to a checkpoint), `log_info.txt`, TensorBoard events under `logs/` and the checkpoints.

TensorBoard is optional: without `torch.utils.tensorboard` scalars go to the log file only and audio is skipped, with one
notice.

Data parallel: `Saver(args, step, rank=r)` with r != 0 counts steps and time like rank 0 but writes NOTHING - no directory, no
`config.yaml`, no log file, no TensorBoard events, no checkpoint - and prints nothing: one rank owns the experiment directory."""
import datetime
import os
import time

import torch
import yaml


def _plain(obj):
    """Nested dict subclasses (DotDict) as plain dicts, so that `yaml.safe_load` reads the dump back."""
    if isinstance(obj, dict):
        return {k: _plain(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_plain(v) for v in obj]
    return obj


class Saver(object):
    def __init__(self, args, initial_global_step=-1, rank=0):
        self.expdir = args.env.expdir
        self.sample_rate = args.data.sampling_rate
        self.global_step = initial_global_step
        self.init_time = self.last_time = time.time()
        self.writes = int(rank) == 0
        self.writer = None
        if not self.writes:
            return
        os.makedirs(self.expdir, exist_ok=True)
        self.path_log_info = os.path.join(self.expdir, "log_info.txt")
        try:
            from torch.utils.tensorboard import SummaryWriter
            self.writer = SummaryWriter(os.path.join(self.expdir, "logs"))
        except ImportError:
            self.writer = None
            self.log_info(" [!] torch.utils.tensorboard is not importable: values go to log_info.txt, audio is not logged")
        with open(os.path.join(self.expdir, "config.yaml"), "w") as fh:
            yaml.safe_dump(_plain(args), fh)

    def log_info(self, msg):
        """A message, or a dict as `key: value` lines (ints with thousands separators), to stdout and `log_info.txt`."""
        if isinstance(msg, dict):
            msg = "\n".join(f"{k}: {v:,}" if isinstance(v, int) else f"{k}: {v}" for k, v in msg.items())
        if not self.writes:
            return
        print(msg)
        with open(self.path_log_info, "a") as fh:
            fh.write(msg + "\n")

    def log_value(self, dict):
        """Scalars at the current step: TensorBoard, or the log file without it."""
        for k, v in dict.items() if self.writes else ():
            if self.writer is not None:
                self.writer.add_scalar(k, v, self.global_step)
            else:
                with open(self.path_log_info, "a") as fh:
                    fh.write(f"[value] step {self.global_step} {k}: {v}\n")

    def log_audio(self, dict):
        """Audio clips at the current step (TensorBoard only)."""
        if self.writer is None:
            return
        for k, v in dict.items():
            self.writer.add_audio(k, v, global_step=self.global_step, sample_rate=self.sample_rate)

    def get_interval_time(self):
        """Seconds since the last call (or construction)."""
        now = time.time()
        interval, self.last_time = now - self.last_time, now
        return interval

    def get_total_time(self):
        """Time since construction as h:mm:ss.d"""
        return str(datetime.timedelta(seconds=time.time() - self.init_time))[:-5]

    def save_model(self, model, optimizer, name="model", postfix=""):
        """`<expdir>/<name>_<postfix>.pt` = {global_step, model: state_dict, optimizer: state_dict} (rank 0 only)."""
        if not self.writes:
            return
        path_pt = os.path.join(self.expdir, f"{name}_{postfix}.pt")
        print(f" [*] model checkpoint saved: {path_pt}")
        torch.save({"global_step": self.global_step, "model": model.state_dict(), "optimizer": optimizer.state_dict()}, path_pt)

    def global_step_increment(self):
        self.global_step += 1
