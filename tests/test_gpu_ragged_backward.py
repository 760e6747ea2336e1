"""Ragged training on the device: `forward(..., n_frames=)` under grad mode, the control network's backward with counts, the
adjoint of the held form and one `training.train_step` on a ragged batch.

The yardstick is always the CPU oracle differentiated by autograd ON EACH ROW ALONE AT ITS OWN LENGTH, the gradients summed
over the rows - never another call of the library.  Gates are the project's own for the same quantities (named at each
assertion).  The padding of units / f0 / volume / phase / noise AND of the upstream gradients is overwritten, once with large
finite garbage and once with NaN; both must give the same bits."""
import numpy as np
import pytest
import torch

import synthetic
from oracle import ctrlnet as OC
from oracle import synth as OS
from ragged_defs import ragged_rss_loss, rel
from test_gpu_ragged import GATE, HOP, _causal_model, poison

pytestmark = pytest.mark.gpu


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _many_lengths():
    """24 rows of up to 172 frames, one of them full: more than 4033 padded rows, from where the prenet convolutions (the
    recomputed forward and the d_t2 adjoint) run the LDS-DMA implicit-im2col GEMM."""
    n = [int(x) for x in _rng(6021).integers(1, 173, size=24)]
    n[5] = 172
    return n


# [80, 12, 1]: 240 padded rows - the K-split launches of the forward, a one-frame row.  [172, 87, 33, 3]: a row without padding,
# 33 = DW_RUN + 1, 87 is no multiple of the 16-frame attention tile, 3 is shorter than the 31-tap depthwise kernel.
# (The backward pass and the fp32 keep-forward choose their kernels by these row counts only: 256 rows for the K-split, 4033
# for the convolutions' GEMM; the fused LayerNorm GEMMs from 8192 rows are inference only.)
SETS = {"ksplit": [80, 12, 1], "whole_k": [172, 87, 33, 3], "dma_conv": _many_lengths()}
CASES = [(s, m, c) for s in ("ksplit", "whole_k") for m in ("per_row", "broadcast", "mix") for c in (False, True)] + \
        [("dma_conv", "per_row", False), ("dma_conv", "mix", True)]


def _poison_rows(x, lengths, kind, per_frame=1):
    x = x.clone()
    for b, n in enumerate(lengths):
        x[b, n * per_frame:] = float("nan") if kind == "nan" else 1e3
    return x


def _gates(got, want, worst_gate, mean_gate, what):
    errs = sorted(((rel(got[n].cpu(), want[n]), n) for n in want), reverse=True)
    print(what, "worst", errs[0], "mean", sum(e for e, _ in errs) / len(errs))
    assert errs[0][0] < worst_gate, (what, errs[:5])
    assert sum(e for e, _ in errs) / len(errs) < mean_gate, (what, errs[:5])


@pytest.mark.parametrize("regime,spk_mode,causal", CASES)
def test_unit2ctrl_ragged_parameter_gradients(dev, lib_path, regime, spk_mode, causal):
    import hipddsp
    lengths = SETS[regime]
    B, Fr = len(lengths), max(lengths)
    model, cfg = _causal_model("CombSub", 31) if causal else synthetic.build_model("CombSub", seed=31)
    u2c = model.unit2ctrl
    inp = synthetic.make_inputs(700 + B, B, Fr, with_noise=False)
    r = _rng(B + Fr)
    inp["phase"] = torch.from_numpy(r.uniform(-np.pi, np.pi, (B, Fr)).astype(np.float32))
    d_ctrl = torch.from_numpy(r.standard_normal((B, Fr, u2c.n_out)).astype(np.float32)) / sum(lengths)
    spk = inp.pop("spk_id")
    spk = spk if spk_mode == "per_row" else spk[:1]
    if spk_mode == "per_row":
        spk[1] = spk[0]                                  # two rows of one speaker: their gradients add up
    mix = {3: 0.5, 10: 0.2, 99: 0.3} if spk_mode == "mix" else None
    # the oracle, row by row at the row's own length; autograd adds the rows' gradients up
    sd = {k: v.clone().requires_grad_(v.is_floating_point() and "projection_matrix" not in k) for k, v in u2c.state_dict().items()}
    for b, n in enumerate(lengths):
        out = OC.unit2control(sd, inp["units"][b:b + 1, :n], inp["f0"][b:b + 1, :n], inp["phase"][b:b + 1, :n],
                              inp["volume"][b:b + 1, :n], spk[b:b + 1] if spk_mode == "per_row" else spk, mix,
                              u2c.output_splits, return_flat=True, causal=causal)
        (out * d_ctrl[b:b + 1, :n]).sum().backward()
    want = {k: v.grad for k, v in sd.items() if v.requires_grad}
    model = model.to(dev)
    names = {n: p for n, p in model.unit2ctrl.named_parameters()}
    assert set(names) == set(want)
    c = hipddsp.context_for(dev)
    first = None
    for kind in ("garbage", "nan"):
        d = {k: v.to(dev) for k, v in poison(inp, lengths, kind).items()}
        d["phase"] = _poison_rows(inp["phase"], lengths, kind).to(dev)
        dc = _poison_rows(d_ctrl, lengths, kind).to(dev)
        args = (d["units"], d["f0"], d["phase"], d["volume"], spk.to(dev), mix)
        grads = model.unit2ctrl.backward_flat(*args, dc, n_frames=lengths)              # the forward is re-run inside
        got = {n: grads[p] for n, p in names.items()}
        # gates of test_unit2ctrl_parameter_gradients
        _gates(got, want, 2e-3, 3e-4, (regime, spk_mode, causal, kind, "split-bf16"))
        used = want["spk_embed.weight"].abs().sum(1) > 0
        assert torch.all(got["spk_embed.weight"].cpu()[~used] == 0)
        if first is None:
            first = got
        else:
            for n in got:                                                               # the padding is not read
                assert torch.equal(got[n], first[n]), n
        # the kept form: same bits as the call that recomputes
        n_dev, *held = u2c.hold_ragged(c, lengths, d["units"], d["f0"], d["phase"], d["volume"])
        ctrl, kept = model.unit2ctrl.forward_ragged_keep(c, *held, spk.to(dev), mix, n_dev, hold=False)
        grads_k = model.unit2ctrl.backward_flat(*held, spk.to(dev), mix, c.ragged_frames(dc, n_dev, hold=False), kept=kept,
                                                n_dev=n_dev)
        for n, p in names.items():
            assert torch.equal(grads_k[p], grads[p]), n
        # fp32 products in the backward: the unfused attention adjoint (five launches) and the round-1 weight gradients
        c.set_math(hipddsp.MATH_FP32)
        try:
            g32 = model.unit2ctrl.backward_flat(*args, dc, n_frames=lengths)
            g32k = model.unit2ctrl.backward_flat(*held, spk.to(dev), mix, c.ragged_frames(dc, n_dev, hold=False), kept=kept,
                                                 n_dev=n_dev)
        finally:
            c.set_math(hipddsp.MATH_SPLIT_BF16)
        _gates({n: g32[p] for n, p in names.items()}, want, 2e-3, 3e-4, (regime, spk_mode, causal, kind, "fp32"))
        for n, p in names.items():
            assert torch.equal(g32k[p], g32[p]), n


@pytest.mark.parametrize("C", [1, 1024])
def test_held_form_adjoint_is_exact(ctx, dev, C):
    B, Fr, counts = 3, 7, [7, 1, 4]
    d = torch.from_numpy(_rng(C).standard_normal((B, Fr, C)).astype(np.float32))
    # autograd of the hold written in torch gives the map; its sum is then taken in the kernel's order, frame by frame
    x = torch.zeros(B, Fr, C, requires_grad=True)
    idx = torch.stack([torch.arange(Fr).clamp(max=n - 1) for n in counts])
    held = torch.gather(x, 1, idx[:, :, None].expand(B, Fr, C))
    (held * d).sum().backward()
    want = torch.zeros_like(d)
    for b, n in enumerate(counts):
        want[b, :n] = d[b, :n]
        for i in range(n, Fr):
            want[b, n - 1] = want[b, n - 1] + d[b, i]
    assert torch.allclose(want, x.grad, rtol=1e-6, atol=1e-6)
    got = ctx.ragged_frames_adjoint_(d.to(dev).clone(), ctx.ragged_counts(counts)).cpu()
    assert torch.equal(got, want)
    if C == 1:
        got2 = ctx.ragged_frames_adjoint_(d[:, :, 0].to(dev).contiguous(), ctx.ragged_counts(counts)).cpu()
        assert torch.equal(got2, want[:, :, 0])


def _oracle_rows_grad(kind, sd0, cfg, inp, lengths, infer, weights):
    """Per-row oracle forwards at the rows' own lengths under autograd; loss = the linear functional `weights` of the three
    outputs, cropped to the row.  -> (rows' signals, {parameter: summed gradient})."""
    params = {k: v.clone().requires_grad_(True) for k, v in sd0.items()
              if v.is_floating_point() and "projection_matrix" not in k and k not in ("window",)}
    sd = dict(sd0)
    sd.update(params)
    sigs = []
    for b, n in enumerate(lengths):
        sig, _, (hm, nz), _ = OS.FORWARD[kind](sd, cfg, inp["units"][b:b + 1, :n], inp["f0"][b:b + 1, :n],
                                               inp["volume"][b:b + 1, :n], inp["spk_id"][b:b + 1], infer=infer,
                                               noise=inp["noise"][b:b + 1, :n * HOP])
        loss = sum((o[0] * w[b, :n * HOP]).sum() for o, w in zip((sig, hm, nz), weights))
        loss.backward()
        sigs.append(sig[0].detach())
    return sigs, {k: v.grad for k, v in params.items()}


MODELS = [("CombSub", False, [40, 17, 1], True), ("Sins", False, [40, 17, 1], True), ("CombSubFast", False, [40, 17, 1], True),
          ("Sins256", False, [20, 7, 1], True), ("CombSub", True, [40, 17, 1], True), ("CombSub", False, [24, 9, 2], False)]


@pytest.mark.parametrize("name,causal,lengths,infer", MODELS)
def test_model_ragged_gradients(dev, lib_path, name, causal, lengths, infer):
    B, Fr = len(lengths), max(lengths)
    model, cfg = _causal_model(name, 13) if causal else synthetic.build_model(name, seed=13)
    inp = synthetic.make_inputs(42 + Fr, B, Fr)
    r = _rng(77)
    weights = [torch.from_numpy(r.standard_normal((B, Fr * HOP)).astype(np.float32)) / (sum(lengths) * HOP) for _ in range(3)]
    sigs, want = _oracle_rows_grad(cfg["type"], model.state_dict(), cfg, inp, lengths, infer, weights)
    model = model.to(dev).train()
    first = None
    for kind in ("garbage", "nan"):
        d = {k: v.to(dev) for k, v in poison(inp, lengths, kind).items()}
        w = [_poison_rows(x, lengths, kind, HOP).to(dev) for x in weights]
        model.zero_grad()
        sig, _, (hm, nz) = model(d["units"], d["f0"], d["volume"], d["spk_id"], infer=infer, noise=d["noise"], n_frames=lengths)
        # the forward keeps the ragged contract (gate of tests/test_gpu_ragged.py; infer=False integrates the phase in fp32)
        for b, n in enumerate(lengths):
            e = float((sig[b, :n * HOP].detach().cpu() - sigs[b]).pow(2).mean().sqrt())
            assert e < (GATE if infer else 5e-3), (b, e)
            assert torch.count_nonzero(sig[b, n * HOP:]) == 0
        # (a product with the poisoned weights: the value of this sum is NaN, its gradient is the weights themselves)
        (sig * w[0] + hm * w[1] + nz * w[2]).sum().backward()
        got = {n: p.grad.clone() for n, p in model.named_parameters()}
        assert set(got) == set(want)
        if infer:   # gates of test_gradients_exact_phase
            _gates(got, want, 2e-2, 5e-3, (name, causal, kind))
        else:       # gates of test_combsub_train_step_matches_autograd
            _gates(got, want, 1e-1, 3e-2, (name, causal, kind))
        if first is None:
            first = got
        else:
            for n in got:
                assert torch.equal(got[n], first[n]), n


def test_ragged_train_step_matches_autograd(dev, lib_path):
    import training
    from ddsp.loss import RSSLoss
    lengths, scales = [24, 9, 2], [300, 777, 1531, 2047]
    B, Fr = len(lengths), max(lengths)
    model, cfg = synthetic.build_model("CombSub", seed=13)
    inp = synthetic.make_inputs(555 + Fr, B, Fr)
    target = torch.from_numpy((0.1 * _rng(9).standard_normal((B, Fr * HOP))).astype(np.float32))
    # the oracle step: the rows' own forwards, the loss of tests/ragged_defs.py over the padded batch, torch's AdamW
    params = {k: v.clone().requires_grad_(True) for k, v in model.state_dict().items()
              if v.is_floating_point() and "projection_matrix" not in k and k not in ("window",)}
    sd = dict(model.state_dict())
    sd.update(params)
    rows = []
    for b, n in enumerate(lengths):
        sig = OS.FORWARD["CombSub"](sd, cfg, inp["units"][b:b + 1, :n], inp["f0"][b:b + 1, :n], inp["volume"][b:b + 1, :n],
                                    inp["spk_id"][b:b + 1], infer=False, noise=inp["noise"][b:b + 1, :n * HOP])[0]
        rows.append(torch.nn.functional.pad(sig[0], (0, (Fr - n) * HOP)))
    loss_o = ragged_rss_loss(torch.stack(rows), target, [n * HOP for n in lengths], scales)
    loss_o.backward()
    opt_o = torch.optim.AdamW(list(params.values()), lr=5e-4, weight_decay=0.0)
    grads_o = {k: v.grad.clone() for k, v in params.items()}
    before = {k: v.detach().clone() for k, v in params.items()}
    opt_o.step()

    model = model.to(dev).train()
    opt = training.AdamW(model.parameters(), lr=5e-4, weight_decay=0.0)
    crit = RSSLoss(256, 2048, 4, device=dev)
    batch = {k: v.to(dev) for k, v in poison(inp, lengths, "nan").items()}
    batch["audio"] = _poison_rows(target, lengths, "nan", HOP).to(dev)
    batch["n_frames"] = lengths
    loss = training.train_step(model, opt, crit, batch, scales=scales)
    # gates of test_combsub_train_step_matches_autograd
    assert abs(float(loss) - float(loss_o)) < 2e-4 * abs(float(loss_o)), (float(loss), float(loss_o))
    _gates({n: p.grad for n, p in model.named_parameters()}, grads_o, 1e-1, 3e-2, "train_step")
    for name, p in model.named_parameters():
        d_got = p.detach().cpu() - before[name]
        d_want = params[name].detach() - before[name]
        if float(d_want.abs().max()) == 0.0:
            continue
        cos = float((d_got.double() * d_want.double()).sum() / (d_got.double().norm() * d_want.double().norm() + 1e-30))
        assert cos > 0.95, (name, cos)
        assert abs(float(d_got.abs().mean()) / float(d_want.abs().mean()) - 1.0) < 0.05, name
