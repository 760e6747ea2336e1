"""Grouped filter synthesis (`ddsp_fir_from_ctrl_group`: one activation launch, one grouped inverse-DFT launch over a tile table,
csrc/gemm_group.h) against the single `ddsp_fir_from_ctrl` calls on the same control matrix: the same bits in every filter.  The
order of the partial sums of a tap does not depend on the tile or on the launch it is formed in, so no tolerance is involved.

Shapes: the grouped form starts at 8192 rows.  8256 = 48 x 172 frames is 129 whole row tiles of 64 (129 % 8 = 1: one leftover row
block dealt round-robin over the XCDs); 8192 + 37 ends in a ragged row tile; 300 rows, fp32 products and an n_mag that is no
multiple of 8 take the single calls inside the grouped entry."""
import numpy as np
import pytest
import torch

import hipddsp
from hipddsp import FIR_ALLPASS, FIR_DYNAMIC, FIR_STATIC

pytestmark = pytest.mark.gpu

SR = 44100
COMBSUB = [(FIR_ALLPASS, 0, 256), (FIR_DYNAMIC, 256, 512), (FIR_STATIC, 768, 256)]    # ctrl: 1024 columns
SINS = [(FIR_ALLPASS, 128, 256), (FIR_STATIC, 384, 256)]                              # ctrl: 128 amplitudes + 512


def _inputs(dev, rows, ld, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    ctrl = torch.from_numpy((rng.standard_normal((rows, ld)) * 0.7).astype(np.float32)).to(dev)
    f0 = rng.uniform(80.0, 800.0, rows).astype(np.float32)
    f0[::7] = 0.0       # unvoiced frames: the dynamic window's half width is 1.5 sr / 1e-3
    return ctrl, torch.from_numpy(f0).to(dev)


def _both(ctx, dev, rows, problems, ld, seed=0):
    ctrl, f0 = _inputs(dev, rows, ld, seed)
    single = [ctx.fir_from_ctrl(mode, ctrl, col, n_mag, rows, SR, f0 if mode == FIR_DYNAMIC else None)
              for mode, col, n_mag in problems]
    grouped = ctx.fir_from_ctrl_group(ctrl, problems, rows, SR, f0)
    torch.cuda.synchronize()
    return single, grouped


def _assert_same_bits(single, grouped):
    assert len(single) == len(grouped)
    for a, b in zip(single, grouped):
        assert a.shape == b.shape
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 1e-3
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("rows,problems,ld", [(8256, COMBSUB, 1024), (8192 + 37, COMBSUB, 1024), (8256, SINS, 640)],
                         ids=["8256x3", "8229x3-ragged-tile", "8256x2-sins"])
def test_grouped_call_writes_the_bits_of_the_single_calls(ctx, dev, rows, problems, ld):
    _assert_same_bits(*_both(ctx, dev, rows, problems, ld, seed=rows + len(problems)))


def test_two_launches(ctx, dev):
    """8256 rows: the single calls are three activation and three inverse-DFT launches, the grouped call one of each (the
    source filter's product is part of the grouped launch, on 64 x 64 tiles like the other two)."""
    rows = 8256
    ctrl, f0 = _inputs(dev, rows, 1024, 3)
    fams = ["fir_act", "fir_dft_gemm"]
    ctx.fir_from_ctrl_group(ctrl, COMBSUB, rows, SR, f0)      # (tables built outside the brackets)
    ctx.profile_begin(fams)
    for mode, col, n_mag in COMBSUB:
        ctx.fir_from_ctrl(mode, ctrl, col, n_mag, rows, SR, f0 if mode == FIR_DYNAMIC else None)
    apart = ctx.profile_end()
    ctx.profile_begin(fams)
    ctx.fir_from_ctrl_group(ctrl, COMBSUB, rows, SR, f0)
    grouped = ctx.profile_end()
    assert [apart[f]["launches"] for f in fams] == [3, 3]
    assert [grouped[f]["launches"] for f in fams] == [1, 1]
    for f in fams:      # the figures the brackets report are the sums of the single calls'
        assert grouped[f]["flops_total"] == apart[f]["flops_total"] and grouped[f]["bytes_total"] == apart[f]["bytes_total"]


def test_small_batch_takes_the_single_calls(ctx, dev):
    single, grouped = _both(ctx, dev, 300, COMBSUB, 1024, seed=4)
    _assert_same_bits(single, grouped)


def test_fp32_products_take_the_single_calls(ctx, dev):
    ctx.set_math(hipddsp.MATH_FP32)
    try:
        single, grouped = _both(ctx, dev, 8256, COMBSUB, 1024, seed=5)
    finally:
        ctx.set_math(hipddsp.MATH_SPLIT_BF16)
    _assert_same_bits(single, grouped)


def test_n_mag_off_the_group_of_8_takes_the_single_calls(ctx, dev):
    problems = [(FIR_ALLPASS, 0, 65), (FIR_DYNAMIC, 256, 512), (FIR_STATIC, 768, 252)]
    rows = 8256
    ctrl, f0 = _inputs(dev, rows, 1024, 6)
    ctx.profile_begin(["fir_act"])
    grouped = ctx.fir_from_ctrl_group(ctrl, problems, rows, SR, f0)
    assert ctx.profile_end()["fir_act"]["launches"] == 3
    single = [ctx.fir_from_ctrl(mode, ctrl, col, n_mag, rows, SR, f0 if mode == FIR_DYNAMIC else None)
              for mode, col, n_mag in problems]
    _assert_same_bits(single, grouped)


def test_arguments_are_checked(ctx, dev):
    ctrl, f0 = _inputs(dev, 16, 1024, 7)
    with pytest.raises(Exception):
        ctx.fir_from_ctrl_group(ctrl, [(FIR_STATIC, 900, 256)], 16, SR)           # columns past the row
    with pytest.raises(Exception):
        ctx.fir_from_ctrl_group(ctrl, [(FIR_DYNAMIC, 0, 256)], 16, SR, None)      # dynamic window without f0
    with pytest.raises(Exception):
        ctx.fir_from_ctrl_group(ctrl, COMBSUB + [(FIR_STATIC, 0, 256)], 16, SR, f0)


def test_render_chain_uses_the_grouped_call(dev, ctx):
    """A CombSub forward at 48 x 172 frames: the filter families hold one launch each, and the signal is the one of the same
    forward with the filters made one by one."""
    import synthetic
    model, _ = synthetic.build_model("CombSub", seed=5, device=dev)
    inp = {k: v.to(dev) for k, v in synthetic.make_inputs(11, 48, 172, with_noise=False).items()}
    args = (inp["units"], inp["f0"], inp["volume"], inp["spk_id"])
    with torch.no_grad():
        ctx.profile_begin(["fir_act", "fir_dft_gemm"])
        sig, _, (harm, noise) = model(*args, noise_seed=9)
        prof = ctx.profile_end()
        assert [prof[f]["launches"] for f in ("fir_act", "fir_dft_gemm")] == [1, 1]
        floor, type(model)._GROUP_MIN_ROWS = type(model)._GROUP_MIN_ROWS, 1 << 30
        try:
            sig1, _, (harm1, noise1) = model(*args, noise_seed=9)
        finally:
            type(model)._GROUP_MIN_ROWS = floor
    for a, b in ((sig, sig1), (harm, harm1), (noise, noise1)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
