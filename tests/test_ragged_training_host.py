"""Ragged training, host side (no GPU): the checks that run before anything is launched."""
import pytest
import torch

import synthetic


def test_ragged_call_under_grad_is_no_longer_refused():
    """CPU tensors: on a model in training mode a ragged call under grad mode gets past the host checks to the 'HIP device
    only' RuntimeError (an eval-mode model keeps its refusal: tests/test_ragged_host.py)."""
    model, cfg = synthetic.build_model("CombSub", seed=3)
    model.train()
    inp = synthetic.make_inputs(5, 3, 8)
    assert model.unit2ctrl.wants_grad()
    assert model.unit2ctrl.check_ragged([8, 3, 1], 3, 8) == [8, 3, 1]
    with pytest.raises(RuntimeError, match="HIP device"):
        model(inp["units"], inp["f0"], inp["volume"], inp["spk_id"], n_frames=[8, 3, 1])
    with pytest.raises(ValueError):
        model(inp["units"], inp["f0"], inp["volume"], inp["spk_id"], n_frames=[8, 3, 9])


def test_spk_mix_rows_under_grad_is_still_refused():
    model, cfg = synthetic.build_model("CombSub", seed=3)
    inp = synthetic.make_inputs(5, 3, 8)
    rows = (torch.ones(3, 1, dtype=torch.int32), torch.ones(3, 1))
    with pytest.raises(NotImplementedError, match="inference only"):
        model(inp["units"], inp["f0"], inp["volume"], inp["spk_id"], n_frames=[8, 3, 1], spk_mix_rows=rows)
    with pytest.raises(NotImplementedError, match="inference only"):
        model(inp["units"], inp["f0"], inp["volume"], inp["spk_id"], spk_mix_rows=rows)


def test_loss_n_samples_are_checked_on_the_host():
    from ddsp.loss import RSSLoss, SSSLoss
    x = torch.zeros(3, 3072)
    crit = RSSLoss(256, 2048, 2)
    for bad in ([3072, 3072], [3072, 3072, 3073], [3072, 0, 3072], [3072, -5, 3072], [3072, 2.0, 3072], 3072,
                torch.tensor([3072.0, 1.0, 1.0])):
        with pytest.raises(ValueError):
            crit(x, x, n_samples=bad)
        with pytest.raises(ValueError):
            SSSLoss(300)(x, x, n_samples=bad)
    with pytest.raises(ValueError, match="whole frame"):      # every row is shorter than the scale
        SSSLoss(300)(x, x, n_samples=[299, 100, 1])
    crit.set_scales([256, 2047])
    with pytest.raises(ValueError, match="whole frame"):
        crit(x, x, n_samples=[2000, 1500, 290])
    with pytest.raises(RuntimeError, match="HIP device"):     # good counts get to the device check
        SSSLoss(300)(x, x, n_samples=[3072, 1500, 290])


def test_train_step_refuses_ragged_data_parallel():
    import training
    batch = {"units": torch.zeros(2, 4, 256), "n_frames": [4, 2]}
    with pytest.raises(ValueError, match="one process"):
        training.train_step(None, None, None, batch, world=2)
