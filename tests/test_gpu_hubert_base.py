"""The base-form units encoder on the device (`ddsp.hubert.HubertBase` -> ddsp_hubert_base_units; `Units_Encoder('cvec' |
'cvec768')`) against the reference class's fp64 output on the unpadded audio (tests/golden/ref_hubert_base.npz), in both
product modes; the shortest inputs; ragged batches; the QKV operand packed on the device against HuBERT-Soft's `in_proj` with
the same numbers; the prepared-weight invalidation; the `Units_Encoder` drop-in and the real-time chain.

The gates are those of tests/test_gpu_hubert.py: the same kernels through fewer layers."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hubert_base_cases as BC
import hubert_cases as HC
import synthetic
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
GATES = {"fp32": 5e-6, "split": 1e-4}


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLDEN, "ref_hubert_base.npz"))


@pytest.fixture(scope="module")
def fill(fix):
    return BC.fairseq_fill(fix, np.load(os.path.join(GOLDEN, "ref_hubert_soft.npz")))


def _base(sd, dev):
    from ddsp.hubert import HubertBase
    m = HubertBase()
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def model(fill, dev, lib_path):
    return _base(fill[0], dev)


@pytest.fixture(params=["fp32", "split"])
def mode(request, ctx):
    import hipddsp
    prev = ctx.math
    ctx.set_math(hipddsp.MATH_FP32 if request.param == "fp32" else hipddsp.MATH_SPLIT_BF16)
    yield request.param
    ctx.set_math(prev)


@pytest.mark.parametrize("project,key,err", [(False, "hidden9_64", "err32"), (True, "units9_64", "err32u")], ids=["hidden", "units"])
@pytest.mark.parametrize("case", BC.CASES)
def test_layer9_against_reference_fp64(model, fix, mode, case, project, key, err, dev):
    got = model.units(HC.audio(case).unsqueeze(1).to(dev), layer=9, project=project)
    torch.cuda.synchronize()
    want = torch.from_numpy(fix[f"{key}_{case}"])
    assert tuple(got.shape) == tuple(want.shape) and want.shape[-1] == (256 if project else 768)
    e = BC.rel(got, want)
    print(f"{case} {mode} project={project}: relative rms {e:.3e}")
    assert e <= GATES[mode], (f"{case} {mode}: relative rms {e:.3e} (gate {GATES[mode]:.0e}; reference fp32 "
                              f"{float(fix[f'{err}_{case}']):.2e}; transformers vs reference fp64 {float(fix['hf_agree_' + case]):.1e})")


@pytest.mark.parametrize("T", [400, 401, 720])
def test_shortest_inputs_run_with_the_fixture_frame_counts(model, fix, T, dev):
    by = dict(zip(list(HC.FRAME_LENGTHS) + list(BC.EXTRA_FRAME_LENGTHS), list(fix["frames0"]) + list(fix["frames0_extra"])))
    x = HC.audio("short")[:, :T].unsqueeze(1).to(dev)
    for project in (False, True):
        got = model.units(x, project=project)
        torch.cuda.synchronize()
        assert got.shape == (1, int(by[T]), 256 if project else 768) and bool(torch.isfinite(got).all())
        assert float(got.abs().max()) > 0


@pytest.mark.parametrize("project", [False, True], ids=["hidden", "units"])
def test_ragged_rows_equal_their_solo_calls(model, project, dev):
    from ddsp.hubert import HubertBase
    counts = [8000, 400, 5123]
    g = np.random.default_rng(17)
    x = torch.from_numpy((0.1 * g.standard_normal((3, 1, 8000))).astype(np.float32))
    for b, n in enumerate(counts):
        x[b, :, n:] = float("nan")
    x = x.to(dev)
    both = model.units(x, n_samples=counts, project=project)
    solo = [model.units(x[b:b + 1, :, :n].contiguous(), project=project) for b, n in enumerate(counts)]
    torch.cuda.synchronize()
    assert both.shape[1] == HubertBase.frames(8000)
    for b, n in enumerate(counts):
        fr = HubertBase.frames(n)
        assert solo[b].shape[1] == fr
        assert torch.equal(both[b, :fr], solo[b][0]), (b, float((both[b, :fr] - solo[b][0]).abs().max()))
        assert not bool(both[b, fr:].any()) and bool(torch.isfinite(both[b]).all())


def test_packed_qkv_equals_in_proj_of_hubert_soft(model, fill, mode, dev):
    """A HubertSoft holding the same numbers reads q, k, v as the three row blocks of `in_proj`; the base form packs its three
    tensors into that operand on the device.  HubertSoft pads 40 zeros on each side; fed the audio padded so, the base form
    sees the same samples, and everything downstream is the same launches: the hidden states are equal bit for bit."""
    from ddsp.hubert import HubertSoft
    soft = HubertSoft()
    soft.load_state_dict(fill[1], strict=True)
    soft = soft.to(dev).eval()
    x = HC.audio("short").unsqueeze(1).to(dev)
    want = soft.encode(x, layer=9)
    got = model.units(F.pad(x, (40, 40)), layer=9, project=False)
    torch.cuda.synchronize()
    assert torch.equal(got, want), f"max |diff| {float((got - want).abs().max()):.3e}"


def test_writes_to_one_projection_reprepare_the_packed_operand(model, fill, dev):
    x = HC.audio("short").unsqueeze(1).to(dev)
    m = _base(fill[0], dev)
    first = m.units(x)
    assert torch.equal(first, model.units(x))
    with torch.no_grad():
        m.encoder.layers[4].self_attn.k_proj.weight.mul_(0.9)
    after = m.units(x)
    want = _base({k: v.detach().cpu() for k, v in m.state_dict().items()}, dev).units(x)
    w = m.encoder.layers[2].self_attn.v_proj.bias
    w.data.copy_(w.data + 0.05)                       # a write torch does not count: rebind()
    m.rebind()
    again = m.units(x)
    want2 = _base({k: v.detach().cpu() for k, v in m.state_dict().items()}, dev).units(x)
    torch.cuda.synchronize()
    assert not torch.equal(first, after) and torch.equal(after, want)
    assert not torch.equal(again, after) and torch.equal(again, want2)


@pytest.fixture(scope="module")
def encoders(fill, dev, lib_path, tmp_path_factory):
    from ddsp.hubert import HubertSoft  # noqa: F401
    from ddsp.vocoder import Units_Encoder
    d = tmp_path_factory.mktemp("cvec")
    torch.save({"model": fill[0]}, str(d / "cvec.pt"))
    torch.save(fill[1], str(d / "soft.pt"))
    return {"cvec768": Units_Encoder("cvec768", str(d / "cvec.pt"), device=dev), "cvec": Units_Encoder("cvec", str(d / "cvec.pt"), device=dev),
            "hubertsoft": Units_Encoder("hubertsoft", str(d / "soft.pt"), device=dev)}


@pytest.mark.parametrize("name,width", [("cvec768", 768), ("cvec", 256)])
def test_units_encoder_ragged_equals_row_by_row(encoders, name, width, dev):
    enc = encoders[name]
    counts = [30000, 17003]
    g = torch.Generator().manual_seed(5)
    a = (0.1 * torch.randn(2, 30000, generator=g))
    a[1, counts[1]:] = float("nan")
    a = a.to(dev)
    got = enc.encode(a, 44100, 512, n_samples=counts)
    rows = [enc.encode(a[b:b + 1, :n].contiguous(), 44100, 512) for b, n in enumerate(counts)]
    torch.cuda.synchronize()
    assert got.shape == (2, 30000 // 512 + 1, width) and enc.n_unit == width
    for b, n in enumerate(counts):
        fr = n // 512 + 1
        assert rows[b].shape == (1, fr, width)
        assert torch.equal(got[b, :fr], rows[b][0]), (b, float((got[b, :fr] - rows[b][0]).abs().max()))
        assert not bool(got[b, fr:].any())
    assert float(got.abs().max()) > 0


def test_push_audio_with_cvec768_graph_equals_eager(encoders, dev):
    """One real-time block chain from the raw audio with a 768-wide encoder and a model built for it: the HIP graph and the
    eager chain agree bit for bit, and the graph is built as often as the HuBERT-Soft renderer builds its own."""
    import realtime
    model, _ = synthetic.build_model("CombSubFast", seed=47, device=dev, n_unit=768)
    kw = dict(buffer_num=4, spk_id=3, units_encoder=encoders["cvec768"], f0_extractor="ac")
    rg = realtime.StreamRenderer(model, 44100, 0.2, 0.04, dev, use_graph=True, **kw)
    re = realtime.StreamRenderer(model, 44100, 0.2, 0.04, dev, use_graph=False, **kw)
    m256, _ = synthetic.build_model("CombSubFast", seed=47, device=dev)
    rs = realtime.StreamRenderer(m256, 44100, 0.2, 0.04, dev, use_graph=True, buffer_num=4, spk_id=3,
                                 units_encoder=encoders["hubertsoft"], f0_extractor="ac")
    rng = np.random.Generator(np.random.PCG64(91))
    for k in range(2):
        t = (np.arange(rg.block) + k * rg.block) / 44100
        blk = torch.from_numpy((0.2 * np.sin(2 * np.pi * 147.0 * t) + 0.01 * rng.standard_normal(rg.block)).astype(np.float32)).to(dev)
        noise = synthetic.make_inputs(7000 + k, 1, rg.frames)["noise"].to(dev)
        a, b = rg.push_audio(blk, noise=noise), re.push_audio(blk, noise=noise)
        rs.push_audio(blk, noise=noise)
        torch.cuda.synchronize()
        assert rg.last_units.shape == (1, rg.frames, 768)
        assert torch.equal(rg.last_units, re.last_units) and torch.equal(rg.last_f0, re.last_f0)
        assert torch.equal(a, b), (k, float((a - b).abs().max()))
        assert float(a.abs().max()) > 0 and float(rg.last_units.abs().max()) > 0
    assert rg.graph_builds == rs.graph_builds == 1 and re.graph_builds == 0
    with pytest.raises(ValueError, match="768 channels"):
        realtime.StreamRenderer(m256, 44100, 0.2, 0.04, dev, use_graph=False, **kw)
