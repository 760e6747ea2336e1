"""All-pass filter synthesis by symmetry (`ddsp_fir_from_ctrl`, mode ALLPASS): taps k and n-k from the even part E (cos
block of exp(j phi) against the cos table) and the odd part O (sin block against the sin table), taps 0..n/2 only.

The reference is the fp64 evaluation of `irfft(exp(1j * cumsum(pi * tanh(ctrl))))`, rotated by n/2 as the reference's
`frequency_filter` without window does (ddsp/core.py:324-326) - so a zero phase gives the unit impulse at tap n/2, and
"tap k" below is a tap of the rotated response.

Bounds: the maximum absolute error of the PARENT commit (full-length transform, K = 2 n_mag, N = n) on exactly these
inputs, measured on an MI355X, times two - room for another rounding order, not for a lost piece product (whose size is
2^-8 .. 2^-16 of a tap).  The literals are in `PARENT_ERR`; nothing is taken from the code under test."""
import numpy as np
import pytest
import torch

import hipddsp

pytestmark = pytest.mark.gpu

SR = 44100
ALLPASS = 0
# rows: one wave, the edges of the 64- and 128-row tiles, two utterances of 172 frames (more than one block), and one row
# count past the threshold from which the operands are written pre-split (8192 rows, n_mag % 8 == 0)
ROWS = (1, 63, 65, 129, 2 * 172, 8199)
# n_mag: the shipped size, the smallest the entry accepts, and an odd one (blocks padded from 65 to 96 columns, generic
# one-bin-per-lane activation kernel, register-staged GEMM)
N_MAGS = (256, 3, 65)

# max |device - fp64| over ROWS of the parent commit, per (n_mag, math); see the module docstring
PARENT_ERR = {
    (256, hipddsp.MATH_SPLIT_BF16): 9.96e-07,
    (256, hipddsp.MATH_FP32): 5.71e-07,
    (3, hipddsp.MATH_SPLIT_BF16): 3.38e-07,
    (3, hipddsp.MATH_FP32): 3.38e-07,
    (65, hipddsp.MATH_SPLIT_BF16): 4.83e-07,
    (65, hipddsp.MATH_FP32): 4.83e-07,
}


def allpass_ctrl(rows, n_mag):
    """(rows, ld) control matrix; the all-pass columns start at column 8 (a 32-byte offset, as the models' heads have)."""
    rng = np.random.Generator(np.random.PCG64(1000 * n_mag + rows))
    ld = n_mag + 24 if n_mag % 4 == 0 else n_mag + 23
    return torch.from_numpy((rng.standard_normal((rows, ld)) * 0.5).astype(np.float32))


def allpass_ref64(c):
    """fp64 reference of the rotated all-pass impulse responses of the control values c :: (rows, n_mag)."""
    phi = torch.cumsum(np.pi * torch.tanh(c.double()), dim=-1)
    ir = torch.fft.irfft(torch.exp(1j * phi))
    return torch.roll(ir, ir.shape[-1] // 2, dims=-1)


def allpass_dev(ctx, dev, ctrl, n_mag, math):
    ctx.set_math(math)
    try:
        return ctx.fir_from_ctrl(ALLPASS, ctrl.to(dev), 8, n_mag, ctrl.shape[0], SR).cpu()
    finally:
        ctx.set_math(hipddsp.MATH_SPLIT_BF16)


def max_err(ctx, dev, rows, n_mag, math):
    ctrl = allpass_ctrl(rows, n_mag)
    got = allpass_dev(ctx, dev, ctrl, n_mag, math)
    return float((got.double() - allpass_ref64(ctrl[:, 8:8 + n_mag])).abs().max())


@pytest.mark.parametrize("math", [hipddsp.MATH_SPLIT_BF16, hipddsp.MATH_FP32])
@pytest.mark.parametrize("n_mag", N_MAGS)
def test_allpass_vs_fp64(ctx, dev, n_mag, math):
    errs = {rows: max_err(ctx, dev, rows, n_mag, math) for rows in ROWS}
    print(f"all-pass n_mag={n_mag} math={math}: max abs error per row count {errs}")
    assert max(errs.values()) <= 2.0 * PARENT_ERR[(n_mag, math)], errs


@pytest.mark.parametrize("math", [hipddsp.MATH_SPLIT_BF16, hipddsp.MATH_FP32])
@pytest.mark.parametrize("n_mag", N_MAGS)
def test_allpass_zero_phase_is_unit_impulse(ctx, dev, n_mag, math):
    n = 2 * (n_mag - 1)
    ctrl = torch.zeros(5, n_mag + 24 if n_mag % 4 == 0 else n_mag + 23)
    got = allpass_dev(ctx, dev, ctrl, n_mag, math).double()
    assert got.shape == (5, n)
    bound = 2.0 * PARENT_ERR[(n_mag, math)]
    assert (got[:, n // 2] - 1.0).abs().max() <= bound
    rest = got.clone()
    rest[:, n // 2] = 0.0
    assert rest.abs().max() <= bound


# (n_mag, bin) of the single-bin cases, and the parent commit's max |device - fp64| on each of them per math mode: these
# responses are close to a scaled impulse (taps of order 1, not of order 1/sqrt(n) as for random phases), so the error of
# the split-bf16 products is larger in absolute terms than on the random inputs above
BIN_CASES = [(256, 1), (256, 100), (256, 254), (65, 33), (3, 1)]
PARENT_ERR_BIN = {
    (256, 1, hipddsp.MATH_SPLIT_BF16): 2.178e-06,
    (256, 1, hipddsp.MATH_FP32): 1.909e-06,
    (256, 100, hipddsp.MATH_SPLIT_BF16): 1.552e-06,
    (256, 100, hipddsp.MATH_FP32): 2.201e-06,
    (256, 254, hipddsp.MATH_SPLIT_BF16): 7.95e-07,
    (256, 254, hipddsp.MATH_FP32): 6.44e-08,
    (65, 33, hipddsp.MATH_SPLIT_BF16): 5.00e-07,
    (65, 33, hipddsp.MATH_FP32): 5.00e-07,
    (3, 1, hipddsp.MATH_SPLIT_BF16): 3.40e-08,
    (3, 1, hipddsp.MATH_FP32): 3.40e-08,
}


def single_bin_ctrl(n_mag, b):
    ctrl = torch.zeros(3, n_mag + 24 if n_mag % 4 == 0 else n_mag + 23)
    ctrl[0, 8 + b] = 0.4
    ctrl[1, 8 + b] = -0.9
    ctrl[2, 8 + b] = 0.05
    return ctrl


def single_bin_err(ctx, dev, n_mag, b, math):
    ctrl = single_bin_ctrl(n_mag, b)
    got = allpass_dev(ctx, dev, ctrl, n_mag, math)
    return float((got.double() - allpass_ref64(ctrl[:, 8:8 + n_mag])).abs().max())


@pytest.mark.parametrize("math", [hipddsp.MATH_SPLIT_BF16, hipddsp.MATH_FP32])
@pytest.mark.parametrize("n_mag,b", BIN_CASES)
def test_allpass_single_group_delay_bin(ctx, dev, n_mag, b, math):
    """One non-zero group-delay bin b: phi = 0 below b and pi*tanh(c) from b on.  The response is neither even nor odd
    about tap n/2, so a mirrored-store index or a sign slip of the odd part shows in the taps checked by value."""
    n = 2 * (n_mag - 1)
    ctrl = single_bin_ctrl(n_mag, b)
    want = allpass_ref64(ctrl[:, 8:8 + n_mag])
    got = allpass_dev(ctx, dev, ctrl, n_mag, math).double()
    bound = 2.0 * PARENT_ERR_BIN[(n_mag, b, math)]
    print(f"all-pass single bin n_mag={n_mag} b={b} math={math}: max abs error {float((got - want).abs().max()):.3e}")
    taps = sorted({0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 1} & set(range(n)))
    for k in taps:
        assert (got[:, k] - want[:, k]).abs().max() <= bound, k
    # the odd part about tap n/2, (h[k] - h[n-k]) / 2, with its sign: far above the bound where the check is made
    k = torch.arange(1, n // 2)
    odd_want = (want[:, k] - want[:, n - k]) / 2
    odd_got = (got[:, k] - got[:, n - k]) / 2
    big = odd_want.abs() > 8 * bound
    assert big.any()
    assert torch.equal(torch.sign(odd_got[big]), torch.sign(odd_want[big]))
    assert (got - want).abs().max() <= bound
