"""One binding method per operation: the solo shape of each merged `hipddsp.Context` method (the solo C symbol) and its batch
shape with B = 1 (the `_ragged` symbol) give the same bits on the same data.  The post-net methods pass no counts on the batch
side (`n_dev=None`, `rows=(1, None, 1)`); `resample`, `retime_f0` and `align_units`, whose `_ragged` symbols refuse NULL counts,
pass full-length ones.  Shapes: the smallest that reach every kernel choice (the narrow, LDS-DMA and register-staged
convolutions, a fused pair), lengths that are no multiple of a tile."""
import numpy as np
import pytest
import torch

import glue_cases as GC

pytestmark = pytest.mark.gpu


def _randn(dev, *shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def test_nsf_source(ctx, dev):
    L, upp = 7, 8
    g = torch.Generator().manual_seed(1)
    f0 = (150.0 + 500.0 * torch.rand(L, generator=g)).to(dev)
    ri = torch.rand(9, generator=g)
    ri[0] = 0
    ri = ri.to(dev)
    w, b = _randn(dev, 9, seed=2), _randn(dev, 1, seed=3)
    solo = ctx.nsf_source(f0, ri, w, b, upp, 44100, 0.1)
    batch = ctx.nsf_source(f0[None], ri[None], w, b, upp, 44100, 0.1, n_dev=None)
    assert solo.shape == (L * upp,) and batch.shape == (1, L * upp)
    assert bool(solo.abs().max() > 0) and torch.equal(batch[0], solo)
    with pytest.raises(ValueError):
        ctx.nsf_source(f0, ri, w, b, upp, 44100, 0.1, n_dev=ctx.ragged_counts([L]))


def test_nsf_noise_conv(ctx, dev):
    T_src, K, stride, pad, T_out, C = 64, 4, 2, 1, 32, 16
    src, w, b = _randn(dev, T_src, seed=4), _randn(dev, C, K, seed=5), _randn(dev, C, seed=6)
    solo = ctx.nsf_noise_conv(src, w, b, K, stride, pad, T_out)
    batch = ctx.nsf_noise_conv(src[None], w, b, K, stride, pad, T_out)
    assert solo.shape == (T_out, C) and batch.shape == (1 * T_out, C)
    assert bool(solo.abs().max() > 0) and torch.equal(batch, solo)


def test_nsf_post(ctx, dev):
    T, C, K = 40, 16, 7
    x, w, b = _randn(dev, T, C, seed=7), _randn(dev, K * C, seed=8) / np.sqrt(K * C), _randn(dev, 1, seed=9)
    solo = ctx.nsf_post(x, w, b, K, 0.01)
    batch = ctx.nsf_post(x, w, b, K, 0.01, rows=(1, None, 1))
    assert solo.shape == (T,) and batch.shape == (1, T)
    assert bool(solo.abs().max() > 0) and torch.equal(batch[0], solo)


@pytest.mark.parametrize("T,Cin,Cout,k,d,in_slope", [(40, 16, 16, 3, 1, 0.1),      # the narrow kernel
                                                     (40, 32, 64, 3, 3, 1.0),      # the LDS-DMA kernel (no activation on load)
                                                     (40, 12, 20, 5, 1, 0.1)])     # the register-staged kernel
def test_conv1d(ctx, dev, T, Cin, Cout, k, d, in_slope):
    x, w = _randn(dev, T, Cin, seed=10), _randn(dev, Cout, k * Cin, seed=11) / np.sqrt(k * Cin)
    b, res = _randn(dev, Cout, seed=12), _randn(dev, T, Cout, seed=13)
    solo = ctx.conv1d(x, w, b, k, d, in_slope, residual=res, act_slope=0.1)
    batch = ctx.conv1d(x, w, b, k, d, in_slope, residual=res, act_slope=0.1, rows=(1, None, 1))
    for s, r in zip(solo, batch):
        assert s.shape == (T, Cout) and bool(s.abs().max() > 0) and torch.equal(r, s)


def test_conv1d_pair(ctx, dev):
    T, C, k, d = 40, 16, 3, 1
    assert ctx.conv1d_pair_supported(C, k, d)
    x = _randn(dev, T, C, seed=14)
    w1, w2 = (_randn(dev, C, k * C, seed=s) / np.sqrt(k * C) for s in (15, 16))
    b1, b2 = _randn(dev, C, seed=17), _randn(dev, C, seed=18)
    solo = ctx.conv1d_pair(x, w1, b1, w2, b2, k, d, 0.1, want_act=True)
    batch = ctx.conv1d_pair(x, w1, b1, w2, b2, k, d, 0.1, want_act=True, rows=(1, None, 1))
    for s, r in zip(solo, batch):
        assert s.shape == (T, C) and bool(s.abs().max() > 0) and torch.equal(r, s)


def test_resample(ctx, dev):
    x = _randn(dev, 1, 300, seed=19)
    solo = ctx.resample(x, 44100, 16000)
    batch = ctx.resample(x, 44100, 16000, n_dev=ctx.ragged_counts([300]))
    assert solo.shape == batch.shape == (1, 109)
    assert bool(solo.abs().max() > 0) and torch.equal(batch, solo)
    assert torch.equal(ctx.resample(x[0], 44100, 16000), solo[0])


def test_retime_f0(ctx, dev):
    f0 = (100.0 + 400.0 * torch.rand(9, generator=torch.Generator().manual_seed(20))).to(dev)
    steps = (512 / 44100, 1.26, 1.26, 441 / 44100, 13)        # targets run past the last knot
    solo = ctx.retime_f0(f0, *steps)
    batch = ctx.retime_f0(f0[None], *steps, n_src_dev=ctx.ragged_counts([9]), n_dst_dev=ctx.ragged_counts([13]))
    assert solo.shape == (13,) and batch.shape == (1, 13)
    assert bool(solo.min() > 0) and torch.equal(batch[0], solo)
    with pytest.raises(ValueError):
        ctx.retime_f0(f0[None], *steps, n_src_dev=ctx.ragged_counts([9]))


def test_align_units(ctx, dev):
    units = _randn(dev, 1, 5, 8, seed=21)
    solo = ctx.align_units(units, 7, 0.9)                        # the last frames stop at the last unit row
    batch = ctx.align_units(units, 7, 0.9, n_units_dev=ctx.ragged_counts([5]), n_out_dev=ctx.ragged_counts([7]))
    assert solo.shape == batch.shape == (1, 7, 8)
    assert torch.equal(solo[0, 6], units[0, 4]) and torch.equal(batch, solo)
    with pytest.raises(ValueError):
        ctx.align_units(units, 7, 0.9, n_out_dev=ctx.ragged_counts([7]))


def test_generator_whole_row_and_full_count(dev, lib_path):
    """`Generator` on one row: without counts and with `n_frames=[L]` (the same launches, with and without a count array)."""
    from enhancer import AttrDict, Generator
    L = 12
    gen = Generator(AttrDict(GC.NSF_CONFIG), GC.nsf_state_dict()).to(dev)
    mel, f0, ri = GC.nsf_inputs(L=L)
    mel, f0 = mel.to(dev), f0.to(dev)
    whole = gen(mel, f0, rand_ini=ri[0])
    counted = gen(mel, f0, rand_ini=ri[0], n_frames=[L])
    assert whole.shape == (1, 1, L * int(np.prod(GC.NSF_CONFIG["upsample_rates"])))
    assert bool(whole.abs().max() > 0) and torch.equal(counted[0], whole[0])
