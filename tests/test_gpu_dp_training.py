"""Data-parallel training on the device: the loss as one rank's share of a global batch, the gradient scale inside the
optimizer's launch, and two ranks (gloo, both on device 0 - the rehearsal form) through `training.train_step` and
`solver.train`.

Every multi-rank test spawns two child processes (tests/dp_workers.py) with a time limit each; a child that exits non-zero
fails the test and nothing is retried.  Tolerances are the project's own for the same quantities, named at each assertion."""
import numpy as np
import pytest
import torch

import dp_workers as W
from ragged_defs import loss_signals, rel

pytestmark = pytest.mark.gpu

# ---- the loss as a share --------------------------------------------------------------------------------------------------
B, T = 4, 4096
COUNTS = [4096, 2600, 1500, 290]
SCALES = [256, 300, 777, 1531]          # row 3 has a frame at 256 only
PARTS = ([0, 3], [1, 2])


def _call(ctx, xp, xt, rows, dev, global_counts=None, hops=None):
    n = [COUNTS[b] for b in rows]
    return ctx.rss_loss(xp[rows].to(dev), xt[rows].to(dev), SCALES, want_grad=True, hops=hops, n_samples=n,
                        global_n_samples=global_counts)


@pytest.mark.parametrize("overlap", [0, 0.75])
def test_loss_shares_add_up_to_the_batch(ctx, dev, overlap):
    """Rows {0, 3} and {1, 2}, each scored with the four global counts: the two values add up to the four-row call's, and
    every row's gradient is its row of the four-row gradient.  Bounds of tests/test_gpu_loss_ragged.py: 5e-5 relative on the
    value, 4e-3 relative norm on the gradient (its floor; both sides are the library here, so no CPU error widens it)."""
    xp, xt = loss_signals(11, B, T)
    hops = None if overlap == 0 else [int(n * (1 - overlap)) for n in SCALES]
    whole, g_whole = _call(ctx, xp, xt, [0, 1, 2, 3], dev, hops=hops)
    total = 0.0
    for rows in PARTS:
        share, g = _call(ctx, xp, xt, rows, dev, COUNTS, hops=hops)
        total += float(share)
        for j, b in enumerate(rows):
            e = rel(g[j].cpu(), g_whole[b].cpu())
            print("overlap", overlap, "row", b, "gradient", e)
            assert e < 4e-3, (b, e)
            assert torch.count_nonzero(g[j, COUNTS[b]:]) == 0
    e_val = abs(total - float(whole)) / abs(float(whole))
    print("overlap", overlap, "shares", total, "batch", float(whole), "relative", e_val)
    assert e_val < 5e-5


def test_share_of_the_whole_batch_has_the_bits_of_the_ragged_call(ctx, dev):
    xp, xt = loss_signals(12, B, T)
    for hops in (None, [n // 4 for n in SCALES]):
        a = _call(ctx, xp, xt, [0, 1, 2, 3], dev, hops=hops)
        b = _call(ctx, xp, xt, [0, 1, 2, 3], dev, list(COUNTS), hops=hops)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_public_forms_and_a_rank_without_a_frame(dev, lib_path):
    """`RSSLoss` / `SSSLoss` with `global_n_samples=` through autograd; a rank whose only row is shorter than every scale but
    one holds a share of 0 there, and one shorter than all of them a share of exactly 0 with a zero gradient."""
    from ddsp.loss import RSSLoss, SSSLoss
    xp, xt = loss_signals(13, B, T)
    crit = RSSLoss(256, 2048, 4, device=dev)
    crit.set_scales(SCALES)
    whole = float(crit(xp.to(dev), xt.to(dev), n_samples=COUNTS))
    total = 0.0
    for rows in ([0, 1, 2], [3]):
        p = xp[rows].to(dev).requires_grad_(True)
        crit.set_scales(SCALES)
        share = crit(p, xt[rows].to(dev), n_samples=[COUNTS[b] for b in rows], global_n_samples=COUNTS)
        share.backward()
        assert bool(torch.isfinite(p.grad).all())
        total += float(share.detach())
    assert abs(total - whole) < 5e-5 * whole, (total, whole)
    one = SSSLoss(300)(xt.to(dev), xp.to(dev), n_samples=COUNTS)
    parts = [SSSLoss(300)(xt[r].to(dev), xp[r].to(dev), n_samples=[COUNTS[b] for b in r], global_n_samples=COUNTS)
             for r in PARTS]
    assert abs(float(parts[0]) + float(parts[1]) - float(one)) < 5e-5 * float(one)
    # T = 288 < every scale: nothing is launched for this rank
    p = xp[3:4, :288].to(dev).requires_grad_(True)
    crit.set_scales([300, 777])
    share = crit(p, xt[3:4, :288].to(dev), n_samples=[288], global_n_samples=[4096, 288])
    share.backward()
    assert float(share.detach()) == 0.0 and torch.count_nonzero(p.grad) == 0
    with pytest.raises(ValueError, match="whole frame"):
        crit.set_scales([300, 2047])
        crit(xp[2:].to(dev), xt[2:].to(dev), n_samples=COUNTS[2:], global_n_samples=[1500, 290, 2000])


# ---- the gradient scale inside the optimizer's launch -------------------------------------------------------------------
ADAMW_SHAPES = ((7, 3), (2049,), (1,), (300, 70)) * 7          # 28 tensors: two launches of 24 and 4


def _adamw_run(dev, grads, **step_kw):
    import training
    g = torch.Generator().manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in ADAMW_SHAPES]
    opt = training.AdamW(params, lr=1e-3, weight_decay=0.01)
    for step in grads:
        for p, x in zip(params, step):
            p.grad = x.to(dev)
        opt.step(**step_kw)
    return [p.detach().cpu() for p in params] + [opt.state[p][k].cpu() for p in params for k in ("exp_avg", "exp_avg_sq")]


def test_adamw_grad_scale(dev, lib_path):
    """Gradients that are multiples of 2^-10 below 2^4 in magnitude: doubling and halving them is exact in fp32, so
    `step(grad_scale=0.5)` on 2 g computes what `step()` computes on g, bit for bit."""
    gen = torch.Generator().manual_seed(4)
    grads = [[torch.randint(-16384, 16384, s, generator=gen).float() / 1024 for s in ADAMW_SHAPES] for _ in range(2)]
    plain = _adamw_run(dev, grads)
    scaled = _adamw_run(dev, [[2 * x for x in step] for step in grads], grad_scale=0.5)
    one = _adamw_run(dev, grads, grad_scale=1.0)
    for a, b, c in zip(plain, scaled, one):
        assert torch.equal(a, b) and torch.equal(a, c)
    third = _adamw_run(dev, [[3 * x for x in step] for step in grads], grad_scale=1.0 / 3.0)
    assert max(rel(b, a) for a, b in zip(plain, third)) < 1e-5            # (not exact: 1/3 rounds)
    import training
    p = torch.nn.Parameter(torch.zeros(4, device=dev))
    p.grad = torch.ones(4, device=dev)
    with pytest.raises(ValueError, match="finite"):
        training.AdamW([p]).step(grad_scale=float("nan"))


# ---- two ranks ------------------------------------------------------------------------------------------------------------
def _split(flat, dev):
    """The flat bucket as {parameter name: gradient}, in the bucket's order."""
    import synthetic
    model, _ = synthetic.build_model("CombSub", seed=13)
    out, off = {}, 0
    for name, p in model.named_parameters():
        out[name] = torch.as_tensor(flat[off:off + p.numel()])
        off += p.numel()
    assert off == len(flat)
    return out


def _bucket_gates(got, want, what):
    """tests/test_gpu_ragged_backward.py, `test_ragged_train_step_matches_autograd`: the parameter gradients' relative-norm
    gates (worst 1e-1, mean 3e-2) and its 5 % check of the mean magnitude, here over the whole bucket."""
    errs = sorted(((rel(got[n], want[n]), n) for n in want), reverse=True)
    mean = sum(e for e, _ in errs) / len(errs)
    mag = float(torch.cat([g.reshape(-1) for g in got.values()]).abs().mean()) / \
        float(torch.cat([g.reshape(-1) for g in want.values()]).abs().mean())
    print(what, "worst", errs[0], "mean", mean, "mean magnitude ratio", mag)
    assert errs[0][0] < 1e-1 and mean < 3e-2, errs[:5]
    assert abs(mag - 1.0) < 0.05


@pytest.mark.parametrize("mode", ["rect", "ragged"])
def test_two_ranks_one_step(dev, lib_path, mode):
    """rect: equal shards of B = 4; the bucket holds the SUM, so half of it is the one-process gradient and the mean of the rank
    losses the one-process loss.  ragged: RAGGED_COUNTS; the shares add up to the one-process loss and the summed bucket is the
    one-process bucket.  Both ranks hold the same bucket bit for bit, and the same parameters after the step.  The loss bound
    is that file's 2e-4."""
    r0, r1 = W.run_ranks(W.device_step_worker, 2, (mode,), timeout=150)
    loss1, flat1, _ = W.device_step(0, 1, mode, dev)
    loss1, flat1 = float(loss1), flat1.cpu()
    assert r0["buckets_equal"] and r0["params_equal"]
    total = r0["loss"] + r1["loss"]
    got_loss, scale = (0.5 * total, 0.5) if mode == "rect" else (total, 1.0)
    print(mode, "rank losses", r0["loss"], r1["loss"], "one process", loss1)
    assert abs(got_loss - loss1) < 2e-4 * abs(loss1)
    _bucket_gates(_split(scale * torch.from_numpy(r0["bucket"]), dev), _split(flat1, dev), mode)


def test_two_ranks_the_loop(dev, lib_path, tmp_path, monkeypatch):
    """`solver.train`, 4 steps, a validation every 2: rank 0 alone writes, its checkpoints load, the validation loss it logged
    is what one process computes on the saved model (2e-4, tests/test_gpu_trainer.py's bound for `validate`), and both ranks
    end with the same parameters.  Validation renders with in-kernel noise whose seed comes from torch's generator; the ranks
    and this process pin it to one value (W.NOISE_SEED), so that the two sides render the same noise."""
    import hipddsp
    import solver
    monkeypatch.setattr(hipddsp, "seed_from_torch", lambda: W.NOISE_SEED)
    import training
    from logger import utils
    root = str(tmp_path)
    r0, r1 = W.run_ranks(W.loop_worker, 2, (root,), timeout=200)
    exp0, exp1 = tmp_path / "exp_rank0", tmp_path / "exp_rank1"
    assert not exp1.exists()
    for f in ("model_2.pt", "model_4.pt", "model_best.pt", "config.yaml", "log_info.txt"):
        assert (exp0 / f).exists(), f
    assert r0["checksum"] == r1["checksum"]
    val = {step: d["validation/loss"] for step, d in r0["logged"] if "validation/loss" in d}
    assert sorted(val) == [2, 4]
    assert [step for step, d in r0["logged"] if "train/loss" in d] == [2, 4]
    case = W.loop_case(root, dev)
    for step in (2, 4):
        assert torch.load(exp0 / f"model_{step}.pt", weights_only=True)["global_step"] == step
    model = W.loop_model(case.SC, dev)
    opt = training.AdamW(model.parameters())
    step, model, opt = utils.load_model(str(exp0), model, opt, device="cuda")
    assert step == 4
    crit = W.training_loss(case, dev)
    d = {}
    want = solver.validate(case.args, model, crit, case.dataset, batch_frames=40, scales=case.scales, details=d)
    print("rank 0 logged", val[4], "one process", want)
    assert abs(val[4] - want) < 2e-4 * want
    assert sorted(d["names"]) == sorted(str(n) for n in case.SC.load()["names"])
