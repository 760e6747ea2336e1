"""Host side of the training loop (`solver`, `logger`): the target-speaker rule, the f0 map restated in numpy against the
fixture of the reference's run, which checkpoint a resume picks, the checkpoint's layout, and the refusals of validation that
happen before anything is launched.  No GPU."""
import os
import types

import numpy as np
import pytest
import torch

import solver_cases as SC


def test_target_speaker_rule():
    import solver
    assert [solver.target_speaker(s, 1) for s in (1,)] == [1]
    assert [solver.target_speaker(s, 2) for s in (1, 2)] == [1, 1]          # 1 -> 2 % 2 = 0 -> 1 ; 2 -> 3 % 2 = 1
    assert [solver.target_speaker(s, 3) for s in (1, 2, 3)] == [2, 1, 1]    # 2 -> 3 % 3 = 0 -> 1 ; 3 -> 4 % 3 = 1
    z = SC.load()
    assert [solver.target_speaker(s, int(z["n_spk"])) for s in z["spk"]] == [int(t) for t in z["tgt"]]


def test_f0_map_in_numpy_against_the_reference_run():
    import solver
    z = SC.load()
    table = solver.lfo_table(SC.f0_stats(z), int(z["n_spk"]))
    assert table.dtype == np.float32 and not np.isnan(table).any()
    zeros = 0
    for i, (src, tgt) in enumerate(zip(z["spk"], z["tgt"])):
        got = SC.vc_f0_numpy(z[f"f0_{i}"], table[src - 1], table[tgt - 1])
        want = z[f"f0_vc_{i}"]
        assert np.array_equal(got == 0, z[f"f0_{i}"] == 0) and np.array_equal(want == 0, z[f"f0_{i}"] == 0)
        # numpy's and torch's float32 log / exp may differ in the last place, and exp carries an error of its argument
        # (about 7) times the argument's relative error: a few float32 epsilon times 7
        assert np.allclose(got, want, rtol=64 * np.finfo(np.float32).eps, atol=0)
        zeros += int((want == 0).sum())
    assert zeros == sum(len(v) for v in SC.UNVOICED.values())
    assert np.isnan(solver.lfo_table({"1": 5.0}, 2)[1])                     # a speaker without a statistic


def _tiny_model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))


def _args(expdir):
    from logger.utils import DotDict
    return DotDict({"env": {"expdir": str(expdir), "gpu_id": 0}, "data": {"sampling_rate": 44100, "block_size": 512},
                    "model": {"type": "CombSub", "n_spk": 3}, "device": "cpu"})


def test_saver_writes_config_and_checkpoint_layout(tmp_path):
    import training
    import yaml
    from logger.saver import Saver
    args = _args(tmp_path / "exp")
    saver = Saver(args, initial_global_step=41)
    with open(tmp_path / "exp" / "config.yaml") as fh:
        assert yaml.safe_load(fh) == {k: dict(v) if isinstance(v, dict) else v for k, v in args.items()}
    saver.global_step_increment()
    saver.log_info({"steps": 1234567, "note": "x"})
    saver.log_value({"train/loss": 1.5})
    assert "steps: 1,234,567" in open(saver.path_log_info).read()
    assert isinstance(saver.get_interval_time(), float) and isinstance(saver.get_total_time(), str)
    model = _tiny_model()
    ours, theirs = training.AdamW(model.parameters()), torch.optim.AdamW(model.parameters())
    # the optimizer state keys are torch.optim.AdamW's for the same parameters (filled in by hand: the kernel needs a GPU)
    for p in model.parameters():
        p.grad = torch.ones_like(p)
        ours.state[p] = {"step": torch.tensor(1.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    theirs.step()
    sd_o, sd_t = ours.state_dict(), theirs.state_dict()
    assert set(sd_o) == set(sd_t) and set(sd_o["state"]) == set(sd_t["state"])
    for k in sd_t["state"]:
        assert set(sd_o["state"][k]) == set(sd_t["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
    assert {k for k in sd_o["param_groups"][0]} <= {k for k in sd_t["param_groups"][0]}
    saver.save_model(model, ours, postfix="42")
    ckpt = torch.load(tmp_path / "exp" / "model_42.pt", weights_only=True)
    assert set(ckpt) == {"global_step", "model", "optimizer"} and ckpt["global_step"] == 42
    assert set(ckpt["model"]) == set(model.state_dict())
    theirs2 = torch.optim.AdamW(_tiny_model().parameters())
    theirs2.load_state_dict(ckpt["optimizer"])                             # the reference's optimizer accepts the file


def test_load_model_picks_the_highest_step_else_best(tmp_path):
    import training
    from logger import utils
    from logger.saver import Saver
    saver = Saver(_args(tmp_path), initial_global_step=0)
    model = _tiny_model()
    opt = training.AdamW(model.parameters())
    assert utils.load_model(str(tmp_path / "nothing_here"), model, opt)[0] == 0
    assert utils.find_checkpoint(str(tmp_path)) is None                    # a cold start: no .pt yet
    for step, fill in ((0, 7.0), (20, 1.0), (300, 2.0)):
        with torch.no_grad():
            for p in model.parameters():
                p.fill_(fill)
        saver.global_step = step if step else 999
        saver.save_model(model, opt, postfix=str(step) if step else "best")
    fresh = _tiny_model()
    step, fresh, _ = utils.load_model(str(tmp_path), fresh, training.AdamW(fresh.parameters()))
    assert step == 300 and all(bool((p == 2.0).all()) for p in fresh.parameters())        # 300 over 20, numerically
    os.remove(tmp_path / "model_300.pt")
    os.remove(tmp_path / "model_20.pt")
    step, fresh, _ = utils.load_model(str(tmp_path), fresh, training.AdamW(fresh.parameters()))
    assert step == 999 and all(bool((p == 7.0).all()) for p in fresh.parameters())        # `best` only without a number
    assert utils.load_config(str(tmp_path / "config.yaml")).env.expdir == str(tmp_path)
    assert sorted(utils.traverse_dir(str(tmp_path), ".pt", is_pure=True, is_ext=False)) == ["model_best"]


def test_validation_refuses_a_too_short_file_before_anything_runs(tmp_path):
    import solver
    short = types.SimpleNamespace(paths=["1/long", "2/short"], whole=[8, 3], hop_size=512, spk_ids=[1, 2], device="cpu")
    crit = types.SimpleNamespace(fft_max=2048)
    with pytest.raises(ValueError, match="2/short"):                       # 3 * 512 = 1536 < 2048; no model, no file is touched
        solver.validate(_args(tmp_path), None, crit, short)
    solver.check_validation_files(["1/a"], [4], 512, 2048)                 # 2048 samples: just long enough
    with pytest.raises(ValueError, match="speaker 2"):                     # 1 is converted to 2, which has no statistic
        solver.check_validation_files(["1/a"], [4], 512, 2048, [1], solver.lfo_table({"1": 5.0}, 3))
