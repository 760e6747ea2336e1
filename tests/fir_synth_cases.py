"""The cases, float64 truths and arithmetic restatements of tests/test_fir_synth_cases_host.py (CPU) and
tests/test_gpu_fir_synth.py (device): filter synthesis, `ddsp_fir_from_ctrl` and its adjoint `ddsp_fir_from_ctrl_bwd`
(csrc/fir_synth.hip).  CPU only; nothing here needs a device or the built library.

Three evaluations of every case, all from the same fp32 inputs:

  ir64     the truth: `oracle.dsp.fir_from_response` in float64.  All-pass: the phase is formed as the kernel and ATen form it (an
           fp64 running sum of the fp32 increments pi_f * tanh, rounded to fp32 per bin), so the truth measures the products and
           not the cumsum convention.
  ir32     the device's fp32 arithmetic restated: activation in fp32, the inverse DFT as a float32 matmul against the fp32 table
           (closed formula in fp64, rounded once; the n/2 rotation and the static Hann folded in, taps 0..n/2, csrc/tables.hip),
           mirrored to taps n/2+1..n-1 (all-pass: cos and sin blocks summed apart, e + o and e - o), the dynamic window in fp32
           in the reference's order of operations.
  irsplit  the same with split-bf16 products: both operands as bf16 hi and lo = bf16(x - hi), the product hi.hi + hi.lo + lo.hi
           accumulated in fp64 and rounded to fp32.

`figures(x, x64)` is the measure, three ways: relative 2-norm over the case, max-abs over the case, the largest relative 2-norm
of a row.  E32 = figures(ir32, ir64) and Esplit = figures(irsplit, ir64) are each arithmetic's own error, from references alone;
the device tests bound the device's figures by 16 x the matching one.  The adjoint has the same three: `d64` is autograd through
the float64 evaluation for a fixed upstream gradient g, `d32` and `dsplit` autograd through the restatements (the split product's
own adjoint is a split product of the gradient with the transposed table).  `win64` (rows, n) is the dynamic window in fp64
(`window64`: the cancellation-free form, so that it is good to an fp32 ulp of every weight).

The dynamic window zeroes w > 1 BEFORE the cosine (ddsp/core.py:292-303): a tap with w just above 1 has weight 1, one just below
about 0, so two correct evaluations that round w differently can disagree by a whole tap.  `_f0_track` keeps every row away
from that: while a row has a tap with |(k - n/2) / hw - 1| < 1e-4 its f0 is multiplied by 1.001 (the device's w carries ~2e-7).

Forward cases and the rule of `gemm::launch` (csrc/gemm_f32.h) each one reaches - N = n/2 + 1 = n_mag output columns, K = n_mag
(all-pass 2 * pad32(n_mag)), tiles counted as ceil(rows / bm) * ceil(N / bn) - are listed at FWD_CASES, the backward ones at
BWD_CASES.  Cases are built lazily and shared (`functools.lru_cache`; the forward cache keeps the last two, a 16k-row case
holds 0.3 GB and builds in about a second); nobody writes into what `fwd_case` / `bwd_case` return.
"""
import functools

import numpy as np
import torch

from oracle import dsp as O

SR = 44100
ALLPASS, DYNAMIC, STATIC = 0, 1, 2            # DDSP_FIR_*
MATH_FP32, MATH_SPLIT_BF16 = 0, 3             # DDSP_MATH_*
BOTH = (MATH_FP32, MATH_SPLIT_BF16)
PI32 = float(np.float32(np.pi))               # the kernels' pi_f
SR15 = float(np.float32(1.5 * SR))            # 66150, exact
MARGIN = 1e-4
MODE_NAME = {ALLPASS: "allpass", DYNAMIC: "dynamic", STATIC: "static"}

FWD_CASES = [
    # mode, n_mag, rows, col0, ld, maths                 rule reached (N = 512 unless noted: 8 column tiles of 64)
    # 27 rows: 8 tiles (N = 512) / 4 tiles (N = 256) of 64x64 -> `blocks(64,64) < 256 && K >= 256`, 64x64 on the 4-stage ring
    (DYNAMIC, 512, 27, 8, 536, BOTH),
    (STATIC, 256, 27, 8, 280, BOTH),
    # n_mag = 513: K % 32 != 0 -> frequency-major table, generic `fir_act_kernel`, register-staged 64x64 `launch_tile`, fp32
    # products in either mode (`bf16_ok` false)
    (STATIC, 513, 27, 8, 536, BOTH),
    # 129 rows: 3 x 8 = 24 tiles, 16 < 24 < 128 -> 32x64 two-wave tile; 129 = 4 * 32 + 1, the last row block holds one row
    (DYNAMIC, 512, 129, 8, 536, BOTH),
    # 1000 rows: 16 x 8 = 128 tiles, not < 128 but < 256 -> 64x64 on the 4-stage ring (SMALL_NS)
    (DYNAMIC, 512, 1000, 8, 536, BOTH),
    # ... and N = 256: 16 x 4 = 64 tiles -> the 32x64 two-wave rule
    (STATIC, 256, 1000, 8, 280, BOTH),
    # 2100 rows: 33 x 8 = 264 tiles of 64x64, 17 x 8 = 136 of 128x64 (< 256), N > 256 -> the last DMA rule, 64x64 3-stage
    (DYNAMIC, 512, 2100, 8, 536, BOTH),
    # 4128 = 24 x 172 rows (training): 33 x 8 = 264 tiles of 128x64 (>= 256), 33 x 4 = 132 of 128x128 (< 512) -> 128x64
    (DYNAMIC, 512, 4128, 8, 536, BOTH),
    # ... and N = 256: 65 x 4 = 260 tiles of 64x64 -> `N <= 256 && blocks(64,64) >= 256`, the skinny 64x64 3-stage rule
    (STATIC, 256, 4128, 8, 280, BOTH),
    # 8199 rows: from 8192 on the split mode writes the activations pre-split (`fir_act_exp8` / `fir_act_allpass4`, split = 1)
    # and the product reads both operands split (MATH = 8); fast window; 8199 = 64 * 128 + 7 = 128 * 64 + 7: ragged last tile.
    # Tiles: 65 x 8 = 520 of 128x64 -> 128x64 (N = 512); skinny 64x64 (N = 256, both); the fp32 mode takes the same tiles
    (DYNAMIC, 512, 8199, 8, 536, BOTH),
    (STATIC, 256, 8199, 8, 280, BOTH),
    (ALLPASS, 256, 8199, 8, 280, BOTH),
    # 16300 rows: 128 x 4 = 512 tiles of 128x128 = T128_MIN -> 128x128, no remainder to cut; 16300 = 127 * 128 + 44
    (DYNAMIC, 512, 16300, 8, 536, BOTH),
    # 16400 rows: 129 x 4 = 516 tiles of 128x128, 516 % 512 = 4 -> with fp32 products (no XCD-aware order) the last 4 are cut
    # out and run as 16 sub-tiles of 64x64 (`sub_from` / `parent_tn`).  Split products keep the XCD order and do not cut.
    (DYNAMIC, 512, 16400, 8, 536, (MATH_FP32,)),
    # column block at an odd column of an odd-pitch matrix: not `wide` -> generic `fir_act_kernel` with M % 8 == 0; the product
    # reads the aligned scratch copy: 2 x 4 = 8 tiles, 64x64 4-stage
    (DYNAMIC, 256, 65, 3, 279, BOTH),
    # beyond the issue's table: the same misaligned block from 8192 rows on in split mode is the generic kernel's split = 1
    # branch (`ddsp_split1_group8`, one bin per lane), which no other test reaches; 129 x 4 tiles, skinny 64x64
    (DYNAMIC, 256, 8199, 3, 279, (MATH_SPLIT_BF16,)),
]

BWD_CASES = [
    # mode, n_mag, rows        `repack` = split mode && pad4(n) % 32 == 0 && rows >= 1024
    # 1023: the last row count on the direct path (register-staged fp32 product, rows of d_ir at pitch n)
    (DYNAMIC, 512, 1023), (STATIC, 256, 1023), (ALLPASS, 256, 1023),
    # 1024: the first repacked one (`repack_rows_kernel`, split-bf16 LDS-DMA product); its first 1023 rows are the case above
    (DYNAMIC, 512, 1024), (STATIC, 256, 1024), (ALLPASS, 256, 1024),
    # 4128: n_mag = 512: rows * ldp / 2 = 2113536 > 8192 * 256 and rows * n > 8192 * 256, both grid-stride loops wrap; for
    # n_mag = 256 the repack grid (1056768 threads) does not wrap, the 128x64 / skinny 64x64 tiles are what is new
    (DYNAMIC, 512, 4128), (STATIC, 256, 4128), (ALLPASS, 256, 4128),
    # odd sizes.  pad4(n) is 128 and 1024 here, multiples of 32 both: what keeps these two on the direct path in either
    # arithmetic is the row count (130 < 1024), not the pitch
    (ALLPASS, 65, 130), (STATIC, 513, 130),
    # beyond the issue's list: an odd n_mag that IS repacked, N = 513 output columns (ragged last column tile), K = 1024
    (STATIC, 513, 1024),
]


def fwd_id(c):
    mode, n_mag, rows, col0 = c[:4]
    return "%s%d-r%d%s" % (MODE_NAME[mode], n_mag, rows, "" if col0 == 8 else "-col%d" % col0)


def bwd_id(c):
    return "%s%d-r%d" % (MODE_NAME[c[0]], c[1], c[2])


def bf16_ok(mode, n_mag):
    """`ddsp_fir_from_ctrl`'s own predicate: the sizes whose forward product follows ddsp_ctx_set_math."""
    K = 2 * ((n_mag + 31) // 32 * 32) if mode == ALLPASS else n_mag
    return K % 32 == 0 and (mode != ALLPASS or n_mag % 16 == 0)


def repacked(n_mag, rows, math):
    """`ddsp_fir_from_ctrl_bwd`'s own predicate."""
    ldp = (2 * (n_mag - 1) + 3) // 4 * 4
    return math != MATH_FP32 and ldp % 32 == 0 and rows >= 1024


def figures(x, x64):
    """(relative 2-norm, max-abs, largest per-row relative 2-norm) of x against the float64 x64."""
    d = x.double() - x64
    return (float(d.norm() / x64.norm()), float(d.abs().max()), float((d.norm(dim=1) / x64.norm(dim=1)).max()))


FIGURE_NAMES = ("rel", "max", "row")


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def near_quirk(f0, n):
    """(rows,) bool: the row has a tap whose w = (k - n/2) / hw is within MARGIN of 1 (fp64 from the fp32 f0)."""
    hw = SR15 / (f0.double() + 1e-3)
    j = torch.arange(-(n // 2), n // 2, dtype=torch.float64)
    return ((j[None, :] / hw[:, None] - 1.0).abs() < MARGIN).any(dim=1)


def _f0_track(rng, rows, n):
    f0 = rng.uniform(65.0, 1200.0, rows).astype(np.float32)
    f0[::7] = 0.0                 # unvoiced: half width 1.5 sr / 1e-3, the window is 1 on every tap
    f0[0] = 65.0                  # half width 1017 > n/2: plain raised cosine
    f0[1] = 800.0                 # half width 82.7: taps with w > 1 (weight 1) and with w < -1 (not clamped)
    f0[2] = 1200.0                # half width 55.1: w reaches -9.3, more than four revolutions of cos(pi w)
    f0 = torch.from_numpy(f0)
    for _ in range(64):
        bad = near_quirk(f0, n)
        if not bool(bad.any()):
            return f0
        f0 = torch.where(bad, f0 * np.float32(1.001), f0)
    raise AssertionError("the quirk margin did not settle")


def _inputs(mode, n_mag, rows, col0, ld, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    ctrl = torch.from_numpy((rng.standard_normal((rows, ld)) * 0.5).astype(np.float32))
    f0 = _f0_track(rng, rows, 2 * (n_mag - 1)) if mode == DYNAMIC else None
    return rng, ctrl, f0


# ---- table and products --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(mode, n_mag):
    """fp32 (n_mag, n/2 + 1) inverse-DFT table of taps 0..n/2, frequency-major: T[f][k] = c_f / n cos(2 pi f (k - n/2) / n),
    times hann_periodic(n)[k] for STATIC; ALLPASS -> (cos table, sin table), the latter -c_f / n sin(...), zero at f = 0 and
    f = n_mag - 1 (csrc/tables.hip).  fp64 with the argument reduced in integers, rounded to fp32 once."""
    M, n = n_mag, 2 * (n_mag - 1)
    f = torch.arange(M, dtype=torch.int64)[:, None]
    k = torch.arange(n // 2 + 1, dtype=torch.int64)[None, :]
    ang = 2.0 * np.pi * torch.remainder(f * (k - n // 2), n).double() / n
    cf = torch.full((M, 1), 2.0, dtype=torch.float64)
    cf[0] = cf[M - 1] = 1.0
    tc = cf / n * torch.cos(ang)
    if mode == STATIC:
        tc = tc * (0.5 - 0.5 * torch.cos(2.0 * np.pi * k.double() / n))
    if mode != ALLPASS:
        return tc.float()
    ts = -cf / n * torch.sin(ang)
    ts[0] = 0.0
    ts[M - 1] = 0.0
    return tc.float(), ts.float()


def _mm32(a, t):
    return a @ t


def _split(x):
    hi = x.bfloat16().float()
    return hi.double(), (x - hi).bfloat16().double()


def _split_product(a, t):
    ah, al = _split(a)
    th, tl = _split(t)
    return (ah @ th + ah @ tl + al @ th).float()


class _SplitMM(torch.autograd.Function):
    """a @ t in split-bf16 products; its adjoint w.r.t. a is the split-bf16 product of the gradient with t transposed."""

    @staticmethod
    def forward(ctx, a, t):
        ctx.save_for_backward(t)
        return _split_product(a, t)

    @staticmethod
    def backward(ctx, g):
        (t,) = ctx.saved_tensors
        return _split_product(g, t.t().contiguous()), None


def window(f0, n, dtype):
    """(rows, n) raised cosine of half width 1.5 sr / (f0 + 1e-3) in `dtype`, the reference's order of operations."""
    if dtype == torch.float64:
        hw = SR15 / (f0.double() + 1e-3)
        pi = np.pi
    else:
        hw = torch.tensor(SR15, dtype=torch.float32) / (f0 + torch.tensor(1e-3, dtype=torch.float32))
        pi = PI32
    pos = torch.arange(-(n // 2), n // 2).to(dtype)[None, :] / hw[:, None]
    pos = torch.where(pos > 1, torch.zeros_like(pos), pos)
    return (1 + torch.cos(pi * pos)) / 2


def window64(f0, n):
    """(rows, n) fp64, the same function as `window` written as cos^2(pi w / 2): (1 + cos(pi w)) / 2 cancels near every odd w < 0,
    where the fp64 form above keeps an absolute 1e-16 on weights down to 3e-13 - hundreds of fp32 ulp of such a weight."""
    pos = torch.arange(-(n // 2), n // 2).double()[None, :] / (SR15 / (f0.double() + 1e-3))[:, None]
    pos = torch.where(pos > 1, torch.zeros_like(pos), pos)
    return torch.cos((np.pi / 2) * pos) ** 2


def restate(mode, n_mag, c, f0, mm):
    """The device's evaluation of the control values c (rows, n_mag) fp32 with the product `mm`; differentiable in c."""
    n = 2 * (n_mag - 1)
    if mode == ALLPASS:
        gd = PI32 * torch.tanh(c)
        phi = torch.cumsum(gd.double(), dim=-1).float()
        tc, ts = table(mode, n_mag)
        e, o = mm(torch.cos(phi), tc), mm(torch.sin(phi), ts)
        return torch.cat([e + o, (e - o)[:, 1:n // 2].flip(-1)], dim=-1)
    act = torch.exp(c) * (1.0 / 128.0) if mode == STATIC else torch.exp(c)
    half = mm(act, table(mode, n_mag))
    ir = torch.cat([half, half[:, 1:n // 2].flip(-1)], dim=-1)         # tap n - k = tap k
    return ir * window(f0, n, torch.float32) if mode == DYNAMIC else ir


def response64(mode, c):
    """fp64 response of the fp32 (or, for autograd, fp64) control values c (rows, n_mag)."""
    c = c.double()
    if mode == ALLPASS:
        gd = (PI32 * torch.tanh(c)).float().double()                    # the fp32 increment
        phi = torch.cumsum(gd, dim=-1).float().double()                 # fp64 running sum, rounded to fp32 per bin
        return torch.exp(1j * phi)
    m = torch.exp(c) if mode == DYNAMIC else torch.exp(c) / 128
    return torch.complex(m, torch.zeros_like(m))


def truth64(mode, c, f0):
    hw = None if mode != DYNAMIC else (SR15 / (f0.double() + 1e-3))[None, :, None]
    return O.fir_from_response(response64(mode, c)[None], hann=(mode != ALLPASS), half_width=hw)[0]


def oracle32(mode, c, f0):
    """`oracle.dsp.fir_from_response` in float32, as tests/test_gpu_dsp.py::test_fir_from_ctrl calls it."""
    if mode == ALLPASS:
        resp = torch.exp(1.j * torch.cumsum(np.pi * torch.tanh(c), dim=-1))
    else:
        m = torch.exp(c) if mode == DYNAMIC else torch.exp(c) / 128
        resp = torch.complex(m, torch.zeros_like(m))
    hw = None if mode != DYNAMIC else (1.5 * SR / (f0 + 1e-3))[None, :, None]
    return O.fir_from_response(resp[None], hann=(mode != ALLPASS), half_width=hw)[0]


# ---- cases -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)      # (a 16k-row case holds 0.3 GB: the tests walk the cases in order, both arithmetics of one together)
def fwd_case(mode, n_mag, rows, col0, ld):
    _, ctrl, f0 = _inputs(mode, n_mag, rows, col0, ld, 100000 * mode + 100 * n_mag + rows + 7 * col0)
    c = ctrl[:, col0:col0 + n_mag].contiguous()
    with torch.no_grad():
        k = dict(mode=mode, n_mag=n_mag, n=2 * (n_mag - 1), rows=rows, col0=col0, ctrl=ctrl, f0=f0, ir64=truth64(mode, c, f0),
                 ir32=restate(mode, n_mag, c, f0, _mm32), irsplit=restate(mode, n_mag, c, f0, _SplitMM.apply))
        if mode == DYNAMIC:
            # the unwindowed response of the unvoiced rows (their window is 1 on every tap)
            unv = torch.nonzero(f0 == 0.0).reshape(-1)
            k["unvoiced"] = unv
            k["raw64_unvoiced"] = O.fir_from_response(response64(mode, c[unv])[None], hann=False)[0]
    return k


@functools.lru_cache(maxsize=None)
def bwd_case(mode, n_mag, rows):
    """col0 = 8; ld = n_mag + 24 (n_mag + 23 for the odd sizes).  The 1023-row case is the first 1023 rows of the 1024-row one."""
    col0, ld, base = 8, n_mag + (24 if n_mag % 4 == 0 else 23), (1024 if rows == 1023 else rows)
    n = 2 * (n_mag - 1)
    rng, ctrl, f0 = _inputs(mode, n_mag, base, col0, ld, 900000 + 100000 * mode + 100 * n_mag + base)
    g = torch.from_numpy(rng.standard_normal((base, n)).astype(np.float32))[:rows].contiguous()
    ctrl = ctrl[:rows].contiguous()
    f0 = None if f0 is None else f0[:rows].contiguous()
    c = ctrl[:, col0:col0 + n_mag].contiguous()

    def grad(dtype, fn):
        x = c.to(dtype).clone().requires_grad_(True)
        (fn(x) * g.to(dtype)).sum().backward()
        return x.grad.detach()

    k = dict(mode=mode, n_mag=n_mag, n=n, rows=rows, col0=col0, ctrl=ctrl, f0=f0, g=g,
             d64=grad(torch.float64, lambda x: truth64(mode, x, f0)),
             d32=grad(torch.float32, lambda x: restate(mode, n_mag, x, f0, _mm32)),
             dsplit=grad(torch.float32, lambda x: restate(mode, n_mag, x, f0, _SplitMM.apply)))
    if mode == DYNAMIC:
        k["win64"] = window64(f0, n)
    return k
