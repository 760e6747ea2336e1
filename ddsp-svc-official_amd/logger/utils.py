"""The reference's `logger/utils.py` (`traverse_dir`, `DotDict`, `load_config`, `load_model`): plain host I/O around the
device path.  A checkpoint is `{'global_step', 'model', 'optimizer'}` as `logger.saver.Saver.save_model` writes it - the
reference's layout, so either side resumes the other's files (`training.AdamW` keeps `torch.optim.AdamW`'s state keys)."""
import os

import torch
import yaml

from ddsp.vocoder import DotDict  # noqa: F401  (one class for every config of the package)


def traverse_dir(root_dir, extension, is_pure=False, is_ext=True):
    """Every file under `root_dir` whose name ends with `extension`, in os.walk order: full paths, or paths relative to
    `root_dir` with `is_pure`; `is_ext=False` strips the last extension."""
    found = []
    for cur, _, names in os.walk(root_dir):
        for name in names:
            if not name.endswith(extension):
                continue
            path = os.path.join(cur, name)
            if is_pure:
                path = os.path.relpath(path, root_dir)
            found.append(path if is_ext else os.path.splitext(path)[0])
    return found


def load_config(path_config):
    """A YAML file as a `DotDict`."""
    with open(path_config, "r") as fh:
        return DotDict(yaml.safe_load(fh))


def find_checkpoint(expdir, name="model", postfix=""):
    """The checkpoint `load_model` resumes from: `<expdir>/<name>_<postfix><step>.pt` with the highest numeric step above 0,
    else `<name>_<postfix>best.pt` when `expdir` holds any `<name>_<postfix>*.pt`, else None (a cold start)."""
    prefix = f"{name}_{postfix}"
    if not os.path.isdir(expdir):
        return None
    tails = [f[len(prefix):-3] for f in os.listdir(expdir) if f.startswith(prefix) and f.endswith(".pt")]
    if not tails:
        return None
    step = max([int(t) for t in tails if t.isdigit()], default=0)
    return os.path.join(expdir, f"{prefix}{step if step > 0 else 'best'}.pt")


def load_model(expdir, model, optimizer, name="model", postfix="", device="cpu"):
    """Restores the freshest checkpoint of `expdir` (`find_checkpoint`) into `model` and `optimizer` ->
    (global_step, model, optimizer); (0, model, optimizer) when there is none.  The optimizer's `step` counters are kept on
    the host wherever the file puts them: `training.AdamW` reads them on every step, and a device tensor there would cost a
    synchronisation per step."""
    path_pt = find_checkpoint(expdir, name, postfix)
    global_step = 0
    if path_pt is not None:
        print(" [*] restoring model from", path_pt)
        ckpt = torch.load(path_pt, map_location=torch.device(device), weights_only=True)
        global_step = ckpt["global_step"]
        model.load_state_dict(ckpt["model"])
        optimizer.load_state_dict(ckpt["optimizer"])
        for state in optimizer.state.values():
            if torch.is_tensor(state.get("step")):
                state["step"] = state["step"].cpu()
    return global_step, model, optimizer
