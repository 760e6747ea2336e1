"""Volume extraction and unit alignment at the non-integral hop `block_size * sample_rate / model_rate` of an input at
another rate than the model's (main.py:72,109; gui.py:94) against tests/golden/ref_volume_frac.npz, the outputs of the
reference's own `Volume_Extractor.extract` and `Units_Encoder.encode` alignment (tests/golden/make_golden_rates.py)."""
import os

import numpy as np
import pytest
import torch

import rates_cases as RC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _golden():
    d = np.load(os.path.join(GOLDEN, "ref_volume_frac.npz"))
    return {k: d[k] for k in d.files}


def test_volume_extract_fractional_hop_matches_reference(dev, lib_path):
    from ddsp.vocoder import Volume_Extractor
    g = _golden()
    for i, h in enumerate(RC.VOLUME_HOPS):
        for j in range(len(RC.volume_lengths(h))):
            audio, hop = RC.volume_audio(i, j)
            want = g[f"vol_{i}_{j}"]
            got = Volume_Extractor(hop, device=dev).extract(audio)
            assert got.shape == want.shape and got.dtype == np.float32, (i, j, got.shape, want.shape)
            # the reference means fp32 squares pairwise in fp32, the kernel sums them in fp64: a few fp32 ulps
            assert np.allclose(got, want, rtol=2e-6, atol=0), (i, j, np.abs(got - want).max())
    # batched rows at a fractional hop are independent
    audio, hop = RC.volume_audio(0, 1)
    x = torch.from_numpy(np.stack([audio, audio[::-1].copy()])).to(dev)
    both = Volume_Extractor(hop, device=dev).extract(x)
    assert both.shape == (2, int(len(audio) // hop) + 1)
    assert np.allclose(both[0].cpu().numpy(), g["vol_0_1"], rtol=2e-6, atol=0)


def test_volume_extract_integral_float_hop_is_the_integer_hop(ctx, dev):
    """256.0 and 441.0 give exactly what 256 and 441 give, through `Volume_Extractor`, through `Context.volume_extract`, and
    through the fractional entry point itself (one kernel behind both)."""
    import hipddsp
    from ddsp.vocoder import Volume_Extractor
    for i, h in enumerate(RC.VOLUME_HOPS):
        if not float(h).is_integer():
            continue
        for j in range(len(RC.volume_lengths(h))):
            audio, _ = RC.volume_audio(i, j)
            x = torch.from_numpy(audio).to(dev)[None]
            ref = ctx.volume_extract(x, int(h))
            assert torch.equal(ctx.volume_extract(x, float(h)), ref)
            assert torch.equal(Volume_Extractor(float(h), device=dev).extract(x[0]), ref[0])
            frac = torch.full_like(ref, -1.0)
            ctx.call("ddsp_volume_extract_frac", hipddsp._ptr(x), 1, x.shape[1], float(h), hipddsp._ptr(frac))
            assert torch.equal(frac, ref), (h, j)


def test_align_units_fractional_hop_matches_reference_exactly(dev, lib_path):
    from ddsp.vocoder import align_units
    g = _golden()
    for i in range(len(RC.ALIGN_CASES)):
        units, n = RC.align_input(i)
        got = align_units(units.to(dev), n, RC.ALIGN_SR, RC.ALIGN_HOP).cpu()
        want = torch.from_numpy(g[f"align_{i}"])
        assert got.shape == want.shape, (i, got.shape, want.shape)
        assert torch.equal(got, want), i


def test_volume_extract_fractional_hop_refusals(ctx, dev):
    h = RC.VOLUME_HOPS[0]                                   # pads 278 / 279
    with pytest.raises(ValueError):
        ctx.volume_extract(torch.zeros(1, 279, device=dev), h)
    ok = ctx.volume_extract(torch.ones(1, 280, device=dev), h)
    assert ok.shape == (1, 1) and float(ok[0, 0]) == 1.0
    with pytest.raises(ValueError):
        ctx.volume_extract(torch.zeros(1, 4000, device=dev), 0.5)
    with pytest.raises(ValueError):
        ctx.volume_extract(torch.zeros(1, 4000, device=dev), float("nan"))
