"""Data-parallel training, host side (no GPU): the loss's denominators, the checks of `global_n_samples`, ragged shards, the
silent `Saver` of the other ranks, the per-step seeds, and two gloo ranks through `training.train_step` on unequal shards
with the oracle stand-ins (tests/dp_workers.py)."""
import os

import numpy as np
import pytest
import torch

import dp_workers as W


def _norms(n_samples, n_ffts, hops):
    """A plain restatement: per scale, the cells that exist and the rows that have a frame."""
    out = []
    for N, hop in zip(n_ffts, hops):
        cells = rows = 0
        for n in n_samples:
            frames = 0
            while frames * hop + N <= n:
                frames += 1
            cells += frames * (N // 2 + 1)
            rows += frames > 0
        out.append((cells, rows))
    return out


def test_loss_norms_against_a_restatement():
    import hipddsp
    n_ffts = [256, 300, 777, 2047]
    for counts in ([3072, 1500, 290], [290], [255, 100], [4096, 2600, 1500, 290, 256, 511, 512]):
        for hops in (n_ffts, [n // 4 for n in n_ffts], [1, 299, 5, 2047]):
            assert hipddsp.loss_norms(counts, n_ffts, hops) == _norms(counts, n_ffts, hops), (counts, hops)
        assert hipddsp.loss_norms(counts, n_ffts) == _norms(counts, n_ffts, n_ffts)
    assert hipddsp.loss_norms([290], n_ffts)[1:] == [(0, 0)] * 3             # a row shorter than the scale
    assert hipddsp.loss_norms([255, 100], n_ffts) == [(0, 0)] * 4            # a rank all of whose rows are
    # a rank's numerators meet the global denominators: the ranks' cells add up to the global count
    parts = [hipddsp.loss_norms(c, n_ffts) for c in ([4096, 290], [2600, 1500])]
    whole = hipddsp.loss_norms([4096, 2600, 1500, 290], n_ffts)
    assert [(a[0] + b[0], a[1] + b[1]) for a, b in zip(*parts)] == whole


def test_global_n_samples_are_checked_on_the_host():
    from ddsp.loss import RSSLoss, SSSLoss
    x = torch.zeros(2, 3072)
    crit = RSSLoss(256, 2048, 2)
    good = [3072, 1500, 3072, 290]
    for bad in ([3072, 0, 3072, 290], [3072, -1, 3072, 290], [3072, 2.0, 3072], 3072, torch.tensor([3072.0, 3072.0]),
                [3072], [3072, 1500, 291], [3072, 3072, 9]):
        with pytest.raises(ValueError):
            crit(x, x, n_samples=[3072, 290], global_n_samples=bad)
        with pytest.raises(ValueError):
            SSSLoss(300)(x, x, n_samples=[3072, 290], global_n_samples=bad)
    with pytest.raises(ValueError, match="n_samples"):                       # the global counts come with the local ones
        crit(x, x, global_n_samples=good)
    crit.set_scales([256, 2047])
    with pytest.raises(ValueError, match="whole frame"):                     # no GLOBAL row has a frame at 2047
        crit(x, x, n_samples=[2000, 290], global_n_samples=[2000, 290, 1500])
    crit.set_scales([256, 2047])
    with pytest.raises(RuntimeError, match="HIP device"):                    # this rank has no frame at 2047: allowed
        crit(x, x, n_samples=[2000, 290], global_n_samples=[2000, 290, 3072])
    with pytest.raises(RuntimeError, match="HIP device"):
        SSSLoss(300)(x, x, n_samples=[290, 100], global_n_samples=[290, 100, 300])
    with pytest.raises(RuntimeError, match="HIP device"):                    # a global row longer than the local padding
        SSSLoss(300)(x, x, n_samples=[3072, 290], global_n_samples=[3072, 290, 8000])


def test_ragged_shards_are_a_partition():
    import sharding
    from data_loaders import epoch_plan, shard_whole
    for counts in ([10, 7, 4, 2], [8, 5, 3, 2], [3, 3, 3], [40, 1, 1, 1, 1, 1, 1]):
        for world in (2, 3):
            parts = [shard_whole(counts, r, world) for r in range(world)]
            assert parts == [sharding.RaggedPlan(counts, world).local(r) for r in range(world)]
            assert sorted(sum(parts, [])) == list(range(len(counts)))
            assert all(parts)                                                 # no rank is left without a row
    full = {"units": torch.zeros(4, 10, 3), "f0": torch.zeros(4, 10, 1), "volume": torch.zeros(4, 10), "spk_id": torch.ones(4, 1),
            "noise": torch.zeros(4, 10 * 512), "audio": torch.zeros(4, 10 * 512)}
    shards = [W.ragged_shard(full, [10, 7, 4, 2], r, 2) for r in range(2)]
    assert shards[0]["global_n_frames"] == shards[1]["global_n_frames"] == [10, 7, 4, 2]
    assert sorted(shards[0]["n_frames"] + shards[1]["n_frames"]) == [2, 4, 7, 10]
    assert [s["units"].shape[1] for s in shards] == [max(s["n_frames"]) for s in shards]
    # fixed-length crops: equal shards on every rank, the same number of steps, a short tail trimmed to a multiple of world
    plans = [epoch_plan(11, 4, r, 2, even=True) for r in range(2)]
    assert plans == [[(0, 2), (4, 2), (8, 1)], [(2, 2), (6, 2), (9, 1)]]
    assert [epoch_plan(9, 4, r, 2, even=True) for r in range(2)] == [[(0, 2), (4, 2)], [(2, 2), (6, 2)]]
    assert epoch_plan(11, 4, 1, 2) == [(2, 2), (6, 2), (10, 1)]              # without `even`: as before


def test_saver_of_another_rank_writes_nothing(tmp_path):
    from logger.saver import Saver
    from logger.utils import DotDict
    args = DotDict({"env": {"expdir": str(tmp_path / "exp")}, "data": {"sampling_rate": 44100}})
    saver = Saver(args, initial_global_step=3, rank=1)
    saver.global_step_increment()
    saver.log_info("a line")
    saver.log_info({"n": 1})
    saver.log_value({"train/loss": 1.0})
    saver.log_audio({"a.wav": torch.zeros(1, 8)})
    net = torch.nn.Linear(2, 2)
    saver.save_model(net, torch.optim.AdamW(net.parameters()), postfix="4")
    assert saver.global_step == 4 and saver.get_interval_time() >= 0
    assert not (tmp_path / "exp").exists() and os.listdir(tmp_path) == []
    Saver(args, initial_global_step=3, rank=0).save_model(net, torch.optim.AdamW(net.parameters()), postfix="4")
    assert (tmp_path / "exp" / "model_4.pt").exists() and (tmp_path / "exp" / "config.yaml").exists()


def test_step_seeds():
    import training
    a = training.step_scales(7, 120, 256, 2048, 4)
    assert a == training.step_scales(7, 120, 256, 2048, 4)                   # every rank, and a run resumed at that step
    assert len(a) == 4 and all(256 <= n < 2048 for n in a)
    assert a != training.step_scales(7, 121, 256, 2048, 4) and a != training.step_scales(8, 120, 256, 2048, 4)
    n0, n1 = training.step_noise_seed(7, 120, 0), training.step_noise_seed(7, 120, 1)
    assert n0 != n1 and n0 == training.step_noise_seed(7, 120, 0) and n0 != training.step_noise_seed(7, 121, 0)
    assert 0 <= n0 < 2 ** 62 and 0 <= n1 < 2 ** 62
    torch.manual_seed(1)
    before = torch.randint(0, 1000, (1,))
    torch.manual_seed(1)
    training.step_scales(7, 120, 256, 2048, 4)                               # its own generator: torch's is untouched
    assert torch.equal(before, torch.randint(0, 1000, (1,)))


def test_train_step_asks_for_global_n_frames():
    import training
    batch = {"units": torch.zeros(2, 4, 256), "global_n_frames": [4, 2, 3]}
    with pytest.raises(ValueError, match="n_frames"):
        training.train_step(None, None, None, batch, world=2)
    with pytest.raises(ValueError, match="Ranks"):
        training.Ranks(2, 2)
    assert (training.Ranks.current().rank, training.Ranks.current().world) == (0, 1)


def test_train_step_ragged_shards_equal_one_process():
    """Counts [10, 7, 4, 2] over two gloo ranks (rows {0, 3} and {1, 2}): the shares add up to the one-process loss and the
    summed bucket is the one-process bucket.  Tolerances of tests/test_dist_gloo.py: 1e-5 relative on the loss, 1e-4 relative
    norm on the bucket."""
    counts = [10, 7, 4, 2]
    (loss1, total1, flat1, n1, g1), = W.run_ranks(W.host_train_worker, 1, (counts,), timeout=300)
    (la, ta, fa, na, ga), (lb, tb, fb, nb, gb) = W.run_ranks(W.host_train_worker, 2, (counts,), timeout=300)
    assert ga == gb == counts and sorted(na + nb) == sorted(counts) and sum(na) != sum(counts) != sum(nb)
    assert total1 == loss1
    assert abs(la + lb - loss1) < 1e-5 * abs(loss1), (la, lb, loss1)
    assert abs(ta - loss1) < 1e-5 * abs(loss1) and ta == tb                  # `global_loss`: the same sum on both ranks
    assert np.array_equal(fa, fb)                                            # both ranks hold the same summed gradient
    assert float(np.linalg.norm(fa - flat1) / np.linalg.norm(flat1)) < 1e-4
