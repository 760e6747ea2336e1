"""HuBERT-Soft units encoder on the device (ddsp/hubert.py -> ddsp_hubert_soft_units) against the reference's fp64 output
(tests/golden/ref_hubert_soft.npz), in both product modes; the attention building block against fp64 torch; the
Units_Encoder drop-in; the prepared-weight cache; graph capture."""
import os

import numpy as np
import pytest
import torch

import hubert_cases as HC
from conftest import GOLDEN

FIX = os.path.join(GOLDEN, "ref_hubert_soft.npz")
GATES = {"fp32": 5e-6, "split": 1e-4}


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float(((a - b) ** 2).mean().sqrt() / (b ** 2).mean().sqrt())


@pytest.fixture(scope="module")
def fix():
    return np.load(FIX)


@pytest.fixture(scope="module")
def model(dev):
    from ddsp.hubert import HubertSoft
    m = HubertSoft()
    m.load_state_dict(HC.fill({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
    return m.to(dev).eval()


@pytest.fixture(params=["fp32", "split"])
def mode(request, ctx):
    import hipddsp
    prev = ctx.math
    ctx.set_math(hipddsp.MATH_FP32 if request.param == "fp32" else hipddsp.MATH_SPLIT_BF16)
    yield request.param
    ctx.set_math(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(HC.CASES))
def test_units_against_reference_fp64(model, fix, mode, case, dev):
    u = model.units(HC.audio(case).unsqueeze(1).to(dev))
    torch.cuda.synchronize()
    want = torch.from_numpy(fix[f"units64_{case}"])
    assert tuple(u.shape) == tuple(want.shape)
    err = _rel(u, want)
    assert err <= GATES[mode], f"{case} {mode}: relative rms {err:.3e} (gate {GATES[mode]:.0e}; reference fp32 {float(fix['err32_' + case]):.2e})"


@pytest.mark.gpu
@pytest.mark.parametrize("layer,key", [(-1, "conv64"), (0, "pre64"), (1, "layer0_64")])
def test_intermediates_against_reference_fp64(model, fix, mode, layer, key, dev):
    h = model.encode(HC.audio("short").unsqueeze(1).to(dev), layer=layer)
    torch.cuda.synchronize()
    err = _rel(h, torch.from_numpy(fix[key]))
    assert err <= GATES[mode], f"{key} {mode}: relative rms {err:.3e}"


@pytest.mark.gpu
def test_batch_rows_equal_single_calls(model, mode, dev):
    x = HC.audio("pair").unsqueeze(1).to(dev)
    both = model.units(x)
    rows = [model.units(x[i:i + 1]) for i in range(2)]
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(both[i], rows[i][0]), f"row {i}: max |diff| {float((both[i] - rows[i][0]).abs().max()):.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 7, 64, 225, 1500])
@pytest.mark.parametrize("math", ["fp32", "split"])
def test_softmax_attention_against_fp64(ctx, dev, L, math):
    import hipddsp
    B, H = 2, 12
    g = torch.Generator().manual_seed(L)
    q, k, v = (torch.randn(B * L, H * 64, generator=g) * s for s in (1.0, 1.0, 0.5))
    out = ctx.softmax_attention(q.to(dev), k.to(dev), v.to(dev), B, L, H,
                                math=hipddsp.MATH_FP32 if math == "fp32" else hipddsp.MATH_SPLIT_BF16)
    torch.cuda.synchronize()
    sh = lambda t: t.double().reshape(B, L, H, 64).transpose(1, 2)  # noqa: E731
    want = torch.softmax(sh(q) @ sh(k).transpose(-1, -2) / 8.0, dim=-1) @ sh(v)
    want = want.transpose(1, 2).reshape(B * L, H * 64)
    err = _rel(out, want)
    assert err <= 1e-6, f"L={L} {math}: relative rms {err:.3e}"


def _encoder(model, tmp_path, dev, prefix=True):
    from ddsp.vocoder import Units_Encoder
    sd = {("module." if prefix else "") + k: v.detach().cpu() for k, v in model.state_dict().items()}
    path = str(tmp_path / "hubert-soft.pt")
    torch.save(sd, path)
    return Units_Encoder("hubertsoft", path, device=dev)


@pytest.mark.gpu
def test_units_encoder_16k_against_reference(model, fix, tmp_path, dev, ctx):
    import hipddsp
    prev = ctx.math
    ctx.set_math(hipddsp.MATH_FP32)
    try:
        enc = _encoder(model, tmp_path, dev)
        a = HC.audio("short").to(dev)
        got = enc.encode(a, 16000, HC.ENCODE_HOP)
        units = enc.model(a)
        from ddsp.vocoder import align_units
        again = align_units(units, a.shape[-1], 16000, HC.ENCODE_HOP)
        torch.cuda.synchronize()
    finally:
        ctx.set_math(prev)
    want = torch.from_numpy(fix["encode32"])
    assert tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got, again)
    err = _rel(got, want)
    assert err <= GATES["fp32"] + float(fix["err32_short"]), f"relative rms {err:.3e}"


@pytest.mark.gpu
def test_units_encoder_resamples_and_keeps_a_fractional_hop(model, tmp_path, dev, ctx):
    enc = _encoder(model, tmp_path, dev)
    g = torch.Generator().manual_seed(3)
    a = (0.1 * torch.randn(1, 44100, generator=g)).to(dev)
    hop = 512 * 44100 / 48000
    got = enc.encode(a, 44100, hop)
    res = ctx.resample(a, 44100, 16000, lowpass_filter_width=128)
    units = model.units(res.unsqueeze(1))
    n = int(a.shape[-1] // hop) + 1
    want = ctx.align_units(units, n, (hop / 44100) / (320 / 16000))
    torch.cuda.synchronize()
    assert got.shape == (1, n, 256)
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_checkpoint_without_prefix_loads_too(model, tmp_path, dev):
    enc = _encoder(model, tmp_path, dev, prefix=False)
    x = HC.audio("short").to(dev)
    assert torch.equal(enc.model(x), model.units(x.unsqueeze(1)))


@pytest.mark.gpu
def test_load_state_dict_after_a_forward_reprepares_the_weights(model, dev):
    from ddsp.hubert import HubertSoft
    x = HC.audio("short").unsqueeze(1).to(dev)
    m = HubertSoft().to(dev)
    m.load_state_dict(model.state_dict())
    first = m.units(x)
    new = {k: v * 0.9 if k.endswith("weight_v") or ("conv" in k and k.endswith("weight")) or k.endswith("linear1.weight")
           else v for k, v in model.state_dict().items()}
    m.load_state_dict(new)
    after = m.units(x)
    fresh = HubertSoft().to(dev)
    fresh.load_state_dict(new)
    want = fresh.units(x)
    torch.cuda.synchronize()
    assert not torch.equal(first, after)
    assert torch.equal(after, want)


@pytest.mark.gpu
def test_prepared_weights_follow_in_place_writes_and_models(model, dev):
    """Two models on one context keep their prepared weights apart; an in-place write under no_grad, and a `.data` write
    followed by `rebind()`, reach the next call - each bit for bit what a fresh model computes."""
    from ddsp.hubert import HubertSoft

    def fresh(sd):
        f = HubertSoft().to(dev)
        f.load_state_dict(sd)
        return f.units(x)

    x = HC.audio("short").unsqueeze(1).to(dev)
    m1, m2 = HubertSoft().to(dev), HubertSoft().to(dev)
    m1.load_state_dict(model.state_dict())
    m2.load_state_dict({k: v * 0.9 if k.endswith("weight_v") else v for k, v in model.state_dict().items()})
    u1, u2 = m1.units(x), m2.units(x)
    assert not torch.equal(u1, u2)
    assert torch.equal(m1.units(x), u1) and torch.equal(u1, fresh(m1.state_dict()))
    assert torch.equal(m2.units(x), u2) and torch.equal(u2, fresh(m2.state_dict()))
    with torch.no_grad():
        m1.feature_extractor.conv1.weight.mul_(0.9)
    after = m1.units(x)
    assert not torch.equal(after, u1) and torch.equal(after, fresh(m1.state_dict()))
    w = m1.positional_embedding.conv.weight_g
    w.data.copy_(w.data * 1.1)
    m1.rebind()
    again = m1.units(x)
    assert not torch.equal(again, after) and torch.equal(again, fresh(m1.state_dict()))


@pytest.mark.gpu
def test_graph_capture_replays_bit_identically(model, dev):
    import hipddsp
    x = HC.audio("gui").unsqueeze(1).to(dev)
    gctx = hipddsp.Context(dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s), hipddsp.use_context(gctx):
        eager = model.units(x)
        eager = model.units(x)   # warm-up: scratch arena at size
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = model.units(x)
    gctx.freeze()
    torch.cuda.current_stream(dev).wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager), f"max |diff| {float((out - eager).abs().max()):.3e}"
