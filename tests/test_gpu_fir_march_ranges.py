"""The march kernel's tap-class form (n = 510 and n = 1022: one product stream per step over compile-time shift
ranges) against the generic march kernel of the same tile form, forced by its math code: the two must agree bit for
bit, because per accumulator they issue the same matrix products in the same order."""
import pytest
import torch

from conftest import rms
from oracle import dsp as O
import hipddsp

pytestmark = pytest.mark.gpu

HOP = 512
SPECIAL = hipddsp.FIR_SPLIT_BF16     # math 3: picks the tap-class kernel when n is 510 or 1022
GENERIC = {510: 47, 1022: 46, 512: 47}   # the generic kernel in the shape math 3 picks for that n (<4,1,pair> / <3,2,pair>)

# (n, B, Fr): whole steps in one chunk; a partial last step with a segment beyond the end and frame Fr on filter Fr - 1;
# two chunks (the second block's first frames lie before its chunk, the first block meets m < 0)
SHAPES = [(510, 128, 16), (510, 128, 19), (510, 64, 35), (1022, 128, 12), (1022, 128, 14), (1022, 64, 26)]


def _inputs(n, B, Fr, dev):
    g = torch.Generator().manual_seed(1000 * n + 10 * B + Fr)
    x = (torch.rand(B, Fr * HOP, generator=g) * 2 - 1).to(dev)
    u = torch.rand(B, Fr * HOP, generator=g).to(dev)
    ir = (torch.randn(B, Fr, n, generator=g) / n ** 0.5).to(dev)
    add = torch.randn(B, Fr * HOP, generator=g).to(dev)
    return x, u, ir, add


def _both(ctx, n, audio, ir, B, Fr, **kw):
    a = ctx.ltv_fir(audio, ir, B, Fr, HOP, math=SPECIAL, **kw)
    b = ctx.ltv_fir(audio, ir, B, Fr, HOP, math=GENERIC[n], **kw)
    return a, b


def _same(a, b):
    for got, want in zip(a, b):
        assert (got is None) == (want is None)
        if got is not None:
            assert torch.equal(got, want)


@pytest.mark.parametrize("variant", ["out", "out_sum", "generate", "unit_noise"])
@pytest.mark.parametrize("n,B,Fr", SHAPES)
def test_tap_class_equals_generic(ctx, dev, n, B, Fr, variant):
    x, u, ir, add = _inputs(n, B, Fr, dev)
    if variant == "out":
        a, b = _both(ctx, n, x, ir, B, Fr)
    elif variant == "out_sum":
        a, b = _both(ctx, n, x, ir, B, Fr, add_in=add)
    elif variant == "generate":
        a, b = _both(ctx, n, None, ir, B, Fr, excitation=hipddsp.EXC_GENERATE, noise_seed=11)
    else:
        a, b = _both(ctx, n, u, ir, B, Fr, excitation=hipddsp.EXC_UNIT_NOISE)
    assert float(a[0].abs().max()) > 0
    _same(a, b)


def test_other_tap_counts_keep_the_generic_kernel(ctx, dev):
    n, B, Fr = 512, 128, 16
    x, _, ir, add = _inputs(n, B, Fr, dev)
    a, b = _both(ctx, n, x, ir, B, Fr, add_in=add)
    assert float(a[0].abs().max()) > 0
    _same(a, b)


def test_tap_class_vs_direct(ctx, dev):
    """Tolerance of test_gpu_dsp.py::test_ltv_fir_split_bf16_vs_direct: 1e-5 of the output's rms, 3e-5 of its peak."""
    n, B, Fr = 510, 128, 16
    x, _, ir, _ = _inputs(n, B, Fr, dev)
    want64 = O.ltv_fir_direct(x.cpu(), ir.cpu())
    got, _ = ctx.ltv_fir(x, ir, B, Fr, HOP, math=SPECIAL)
    got = got.cpu()
    scale, peak = rms(want64), float(want64.abs().max())
    assert rms(got.double() - want64) < 1e-5 * scale
    assert (got.double() - want64).abs().max() < 3e-5 * peak
