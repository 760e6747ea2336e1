"""CPU: the cases of tests/fir_synth_cases.py are what tests/test_gpu_fir_synth.py takes them for.

The device tests bound the device's error by 16 x the error of a CPU restatement of the device's arithmetic (E32: fp32 products,
Esplit: split-bf16 products; tests/fir_synth_cases.py).  That means something only while the restatement is right and its error
is rounding-sized.  So, for every case:

  - no tap of any row is within 1e-4 of the window's discontinuity at w = 1, and the fp32 and fp64 windows take the same branch;
  - `ir32` agrees with `oracle.dsp.fir_from_response` on fp32 inputs to 4 x E32 (the table's rotation, Hann fold, mirror and
    even/odd split are right before any device sees them);
  - E32 and Esplit, each as (relative 2-norm, max-abs, largest per-row relative 2-norm), are within 4 x either side of the
    values below; Esplit is above E32 and in the class of the header's "~4e-6 per contraction" (case-wide relative figure
    between 1e-6 and 2e-5); the case-wide relative figure of E32 is between 1e-8 and 1e-5;
  - the same for the adjoint's d32 and dsplit against d64.

MEASURED on the CPU while writing the test, (relative, max-abs, per-row) of E32 and of Esplit: the literals of FWD_MEASURED and
BWD_MEASURED below.  STATIC taps are of order 1e-3 (exp(c) / 128 over n taps under a Hann), hence their small max-abs figures;
the all-pass E32 is larger than the others because its truth forms tanh in fp64 before rounding the increment to fp32, the
restatement (and the device) in fp32: a 1-ulp difference of an increment stays in every later bin's phase.

The fp32 window against `win64`: the reference's own fp32 evaluation of (1 + cos(pi w)) / 2 is up to 1.6e-6 from the fp64 one
(pi_f * w is rounded at |w| up to 9.3, and 1 + cos cancels near odd w), so g * win32 is further than 4 fp32 ulp from g * win64
on 18 % of the elements of the DYNAMIC backward cases.  test_fp32_window_against_win64 records that: it is why the adjoint's
`dyn_window_scale_kernel` forms the weight in fp64 (tests/test_gpu_fir_synth.py::test_dynamic_adjoint_d_ir_within_4_ulp), and
why `win64` itself is the cancellation-free cos^2(pi w / 2): the fp64 (1 + cos(pi w)) / 2 is 487 fp32 ulp off a weight of
3e-13 in the 4128-row case.
"""
import pytest
import torch

import fir_synth_cases as C

FWD_MEASURED = {
    "dynamic512-r27":          ((3.04e-07, 3.47e-07, 4.64e-07), (5.05e-06, 4.70e-06, 5.67e-06)),
    "static256-r27":           ((2.82e-07, 5.63e-09, 6.91e-07), (3.52e-06, 1.01e-08, 4.21e-06)),
    "static513-r27":           ((2.86e-07, 3.24e-09, 4.90e-07), (2.42e-06, 4.60e-09, 2.77e-06)),
    "dynamic512-r129":         ((3.08e-07, 7.21e-07, 6.46e-07), (5.08e-06, 4.85e-06, 5.83e-06)),
    "dynamic512-r1000":        ((2.97e-07, 6.87e-07, 6.50e-07), (5.08e-06, 5.09e-06, 6.01e-06)),
    "static256-r1000":         ((3.01e-07, 6.94e-09, 7.63e-07), (3.56e-06, 1.73e-08, 4.34e-06)),
    "dynamic512-r2100":        ((3.01e-07, 7.84e-07, 6.51e-07), (5.07e-06, 5.11e-06, 6.23e-06)),
    "dynamic512-r4128":        ((2.99e-07, 7.48e-07, 6.74e-07), (5.08e-06, 5.45e-06, 6.05e-06)),
    "static256-r4128":         ((3.02e-07, 8.55e-09, 8.99e-07), (3.57e-06, 1.68e-08, 4.43e-06)),
    "dynamic512-r8199":        ((2.99e-07, 7.75e-07, 6.89e-07), (5.08e-06, 5.45e-06, 6.02e-06)),
    "static256-r8199":         ((3.00e-07, 8.01e-09, 8.90e-07), (3.56e-06, 2.39e-08, 4.58e-06)),
    "allpass256-r8199":        ((8.59e-07, 5.15e-07, 2.85e-06), (3.59e-06, 1.07e-06, 4.44e-06)),
    "dynamic512-r16300":       ((3.00e-07, 7.73e-07, 7.93e-07), (5.08e-06, 5.34e-06, 6.06e-06)),
    "dynamic512-r16400":       ((2.99e-07, 7.94e-07, 7.55e-07), (5.08e-06, 5.49e-06, 6.06e-06)),
    "dynamic256-r65-col3":     ((3.05e-07, 6.89e-07, 5.77e-07), (4.02e-06, 1.62e-06, 5.39e-06)),
    "dynamic256-r8199-col3":   ((3.00e-07, 1.17e-06, 9.11e-07), (3.94e-06, 2.59e-06, 6.24e-06)),
}
BWD_MEASURED = {
    "dynamic512-r1023":        ((3.22e-07, 2.94e-07, 4.92e-07), (3.94e-06, 3.16e-06, 4.90e-06)),
    "static256-r1023":         ((2.02e-07, 1.35e-09, 2.95e-07), (4.23e-06, 1.75e-08, 6.41e-06)),
    "allpass256-r1023":        ((9.82e-07, 1.39e-05, 1.27e-05), (4.25e-06, 5.29e-05, 4.38e-05)),
    "dynamic512-r1024":        ((3.22e-07, 2.94e-07, 4.92e-07), (3.94e-06, 3.16e-06, 4.90e-06)),
    "static256-r1024":         ((2.02e-07, 1.35e-09, 2.95e-07), (4.23e-06, 1.75e-08, 6.41e-06)),
    "allpass256-r1024":        ((9.82e-07, 1.39e-05, 1.27e-05), (4.25e-06, 5.29e-05, 4.38e-05)),
    "dynamic512-r4128":        ((3.22e-07, 3.83e-07, 5.10e-07), (3.94e-06, 3.74e-06, 5.10e-06)),
    "static256-r4128":         ((2.02e-07, 2.19e-09, 3.98e-07), (4.20e-06, 3.11e-08, 7.55e-06)),
    "allpass256-r4128":        ((9.74e-07, 2.61e-05, 1.24e-05), (4.27e-06, 4.92e-05, 4.03e-05)),
    "allpass65-r130":          ((5.51e-07, 8.15e-06, 4.34e-06), (3.54e-06, 3.91e-05, 2.72e-05)),
    "static513-r130":          ((2.54e-07, 1.27e-09, 3.21e-07), (4.18e-06, 1.13e-08, 4.95e-06)),
    "static513-r1024":         ((2.57e-07, 1.54e-09, 3.59e-07), (4.18e-06, 1.60e-08, 5.35e-06)),
}
BAND = 4.0
LO, HI = 1e-8, 1e-5             # relative figures of E32 (tests/test_dsp_stage_cases_host.py)
SPLIT_LO, SPLIT_HI = 1e-6, 2e-5   # relative figures of Esplit: the class of "~4e-6 per contraction"


def _in_band(what, got, pinned):
    for name, g, p in zip(C.FIGURE_NAMES, got, pinned):
        assert p / BAND <= g <= p * BAND, (what, name, g, p)


def _check_figures(what, e32, esplit, pinned):
    print(f"MEASURED {what}: E32 " + " ".join(f"{v:.2e}" for v in e32) + "  Esplit " + " ".join(f"{v:.2e}" for v in esplit))
    _in_band(what + " E32", e32, pinned[0])
    _in_band(what + " Esplit", esplit, pinned[1])
    # the case-wide relative figure (the worst ROW of the all-pass adjoint, whose reverse running sum cancels on some rows,
    # is 1.3e-5 / 4.4e-5: held by its band alone)
    assert LO < e32[0] < HI, (what, e32)
    assert SPLIT_LO < esplit[0] < SPLIT_HI, (what, esplit)
    for a, b in zip(e32, esplit):
        assert b > a, (what, e32, esplit)


def _check_margin(k):
    """No tap within the margin of w = 1 on any row; the fp32 and fp64 evaluations of w take the same branch on every tap."""
    f0, n = k["f0"], k["n"]
    assert f0.dtype == torch.float32 and f0.shape == (k["rows"],)
    assert not bool(C.near_quirk(f0, n).any())
    j = torch.arange(-(n // 2), n // 2)
    hw32 = torch.tensor(C.SR15, dtype=torch.float32) / (f0 + torch.tensor(1e-3, dtype=torch.float32))
    w32 = j.float()[None, :] / hw32[:, None]
    w64 = j.double()[None, :] / (C.SR15 / (f0.double() + 1e-3))[:, None]
    assert torch.equal(w32 > 1, w64 > 1)
    assert float((w64 - 1).abs().min()) >= C.MARGIN
    # the track holds what the cases are there for: unvoiced rows, the three fixed rows, f0 beyond 800 Hz
    assert bool((f0[7::7] == 0.0).all()) and float(f0[0]) == 65.0
    assert 800.0 <= float(f0[1]) < 810.0 and 1200.0 <= float(f0[2]) < 1215.0
    assert bool((w64[1] > 1).any()) and bool((w64[1] < -1).any())
    assert float(w64[2].min()) < -(n // 2) / 55.2          # -9.3 at n = 1022: more than four revolutions of cos(pi w)
    voiced = f0[f0 > 0]
    assert float(voiced.min()) >= 65.0 and float(voiced.max()) <= 1200.0 * 1.001 ** 8


@pytest.mark.parametrize("case", C.FWD_CASES, ids=C.fwd_id)
def test_forward_case(case):
    mode, n_mag, rows, col0, ld, _ = case
    k = C.fwd_case(*case[:5])
    n = 2 * (n_mag - 1)
    assert k["ctrl"].shape == (rows, ld) and col0 + n_mag <= ld
    assert k["ir64"].dtype == torch.float64 and k["ir64"].shape == (rows, n)
    for name in ("ir32", "irsplit"):
        assert k[name].dtype == torch.float32 and k[name].shape == (rows, n) and bool(torch.isfinite(k[name]).all())
    if mode == C.DYNAMIC:
        _check_margin(k)
        assert len(k["unvoiced"]) >= rows // 7 - 1 and k["raw64_unvoiced"].shape == (len(k["unvoiced"]), n)
        # an unvoiced row's window is 1 on every tap (1 - 1.5e-10 at the ends in fp64, 1 in fp32)
        assert C.figures(k["ir64"][k["unvoiced"]], k["raw64_unvoiced"])[2] < 1e-9
    e32, esplit = C.figures(k["ir32"], k["ir64"]), C.figures(k["irsplit"], k["ir64"])
    _check_figures(C.fwd_id(case), e32, esplit, FWD_MEASURED[C.fwd_id(case)])
    # the restatement against the project's oracle at the device's precision
    c = k["ctrl"][:, col0:col0 + n_mag].contiguous()
    o32 = C.oracle32(mode, c, k["f0"])
    assert o32.dtype == torch.float32
    for g, e in zip(C.figures(k["ir32"], o32.double()), e32):
        assert g <= 4.0 * e, (C.fwd_id(case), g, e)


@pytest.mark.parametrize("case", C.BWD_CASES, ids=C.bwd_id)
def test_backward_case(case):
    mode, n_mag, rows = case
    k = C.bwd_case(*case)
    assert k["g"].shape == (rows, 2 * (n_mag - 1)) and k["d64"].shape == (rows, n_mag) and k["d64"].dtype == torch.float64
    for name in ("d32", "dsplit"):
        assert k[name].dtype == torch.float32 and k[name].shape == (rows, n_mag) and bool(torch.isfinite(k[name]).all())
    if mode == C.DYNAMIC:
        _check_margin(k)
        assert k["win64"].shape == k["g"].shape and k["win64"].dtype == torch.float64
        assert float(k["win64"].min()) >= 0.0 and float(k["win64"].max()) <= 1.0
    _check_figures(C.bwd_id(case), C.figures(k["d32"], k["d64"]), C.figures(k["dsplit"], k["d64"]), BWD_MEASURED[C.bwd_id(case)])


@pytest.mark.parametrize("mode,n_mag", [(C.DYNAMIC, 512), (C.STATIC, 256), (C.ALLPASS, 256)])
def test_1023_rows_are_the_first_of_1024(mode, n_mag):
    a, b = C.bwd_case(mode, n_mag, 1023), C.bwd_case(mode, n_mag, 1024)
    for name in ("ctrl", "g", "d64", "f0"):
        if a[name] is not None:
            assert torch.equal(a[name], b[name][:1023]), name


def test_split_adjoint_is_the_transposed_split_product():
    """<g, split(a, t)> differentiates to split(g, t^T): a linear map's adjoint, in the same three-piece arithmetic."""
    gen = torch.Generator().manual_seed(3)
    a = torch.randn(5, 32, generator=gen).requires_grad_(True)
    t, g = torch.randn(32, 9, generator=gen), torch.randn(5, 9, generator=gen)
    (C._SplitMM.apply(a, t) * g).sum().backward()
    want = g.double() @ t.double().t()
    assert C.figures(a.grad, want)[0] < 2e-5 and not torch.equal(a.grad.double(), want)


def test_predicates():
    assert C.bf16_ok(C.DYNAMIC, 512) and C.bf16_ok(C.ALLPASS, 256) and not C.bf16_ok(C.STATIC, 513)
    assert not C.bf16_ok(C.ALLPASS, 65)
    assert C.repacked(512, 1024, C.MATH_SPLIT_BF16) and not C.repacked(512, 1023, C.MATH_SPLIT_BF16)
    assert not C.repacked(512, 4128, C.MATH_FP32) and not C.repacked(65, 130, C.MATH_SPLIT_BF16)
    assert C.repacked(513, 1024, C.MATH_SPLIT_BF16)


def test_fp32_window_against_win64():
    """The reference's window in fp32 against `win64` (module docstring): rounding-sized in absolute terms, not within 4 fp32 ulp
    of each element."""
    k = C.bwd_case(C.DYNAMIC, 512, 1024)
    w32 = C.window(k["f0"], k["n"], torch.float32)
    assert w32.dtype == torch.float32
    assert float((w32.double() - k["win64"]).abs().max()) < 4e-6
    want = k["g"].double() * k["win64"]
    ulp = torch.ldexp(torch.ones_like(want), torch.floor(torch.log2(want.abs().clamp_min(1e-300))) - 23)
    beyond = ((k["g"] * w32).double() - want).abs() > 4 * ulp
    print("MEASURED g * win32 beyond 4 ulp of g * win64:", float(beyond.double().mean()))
    assert 0.05 < float(beyond.double().mean()) < 0.5


@pytest.mark.parametrize("rows", [1024, 4128])
def test_win64_is_the_oracle_s_window(rows):
    """cos^2(pi w / 2) against the oracle's (1 + cos(pi w)) / 2, both in fp64: the same function to 1e-15."""
    k = C.bwd_case(C.DYNAMIC, 512, rows)
    assert float((k["win64"] - C.window(k["f0"], k["n"], torch.float64)).abs().max()) < 1e-15
