"""Stage tests of the sinusoid bank and its adjoint (csrc/sins_bank.hip), the spectral overlap-add and its adjoint
(csrc/spectral_ola.hip) and the two in-kernel noise generators, each entry called directly at the smallest shapes that reach
every branch (tests/dsp_stage_cases.py lists them and what each is there for).

One tolerance rule everywhere.  Each forward output or gradient `got` is compared with the float64 oracle x64, and the bound is
the float32 oracle's own distance x32 from it (E32, computed here from the references alone):

    ||got - x64|| / ||x64||  <=  FACTOR * E32          max|got - x64|  <=  FACTOR * max|x32 - x64|          FACTOR = 16

The device differs from the float32 oracle by rounding only - another FFT factorisation and a float32 twiddle table, two real
spectra packed into one transform, 1-2 ulp expf / sincosf, a 32-step rotation recurrence, another order of the sums - each a
few units of the oracle's own error, while a structural error (a neighbouring frame's filter, a lost conjugate, the window
applied once, a harmonic off by one, a dropped j/hop share, a dropped +1e-7) shows at 1e-3 relative or more.
tests/test_dsp_stage_cases_host.py holds E32 itself between 1e-8 and 1e-5.

MEASURED (MI355X), error / E32 as "relative, max-abs"; the worst of the compared parts (adjoint of the bank: unmasked and
masked entries; adjoint of the OLA: all 1539 columns and the hm, hp, nm blocks):

    stage  case                        forward         adjoint
    bank   B2-Fr3-H150-hop512-col4      0.45,  0.26     0.99,  1.04
    bank   B1-Fr2-H100-hop512-col4      0.48,  0.37     0.80,  1.02
    bank   B2-Fr3-H37-hop1024-col4      0.47,  0.73     1.08,  1.35
    bank   B1-Fr4-H256-hop256-col4      0.48,  0.72     0.92,  0.91
    bank   B2-Fr5-H96-hop64-col4        0.37,  0.30     0.76,  1.18
    bank   B1-Fr1-H128-hop512-col4      0.29,  0.20     0.75,  0.87
    bank   B1-Fr3-H33-hop512-col3       0.51,  0.64     0.52,  0.64
    bank   B1-Fr2-H1-hop512-col4        0.97,  0.81     0.33,  0.33
    ola    B2-Fr1-uniform               1.15,  2.27     1.26,  1.43
    ola    B2-Fr2-uniform               1.26,  2.88     1.34,  1.54
    ola    B1-Fr5-sinc                  3.65,  4.26     3.76,  6.09
    ola    B3-Fr9-uniform               1.28,  2.95     1.38,  1.55
    bank   H2048 (LDS range)            0.36,  0.20     1.07,  1.44

Nothing comes near 16.  The bank is below 1 because it seeds every 32nd harmonic from the same rounded product k * phase as
the oracle and reaches the 31 between by rotation, which does not round k * phase again.  The OLA's largest ratio is the
`sinc_comb` case: the kernel transforms comb + j * noise in one FFT, so the rounding error of the comb's spectrum scales
with the norm of both (the comb's rms there is 0.06, the noise's 0.58), where the oracle transforms the comb alone.
Sins(n_harmonics=100): forward 3.2e-6 rms against the 1e-4 gate; gradients worst 5.2e-4, mean 2.3e-4 (bounds 2e-2, 5e-3).
"""
import numpy as np
import pytest
import torch

import dsp_stage_cases as C

pytestmark = pytest.mark.gpu
SR = C.SR
FACTOR = 16.0
# a case above 16 gets its own factor here, with the reason beside it (none does)
CASE_FACTOR = {}


def _close(what, got, x32, x64, factor=FACTOR):
    """The rule of the module docstring; prints error / E32 (the table above is made of these lines)."""
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == x64.shape and bool(torch.isfinite(got).all()), what
    e32, m32 = C.rel_err(x32, x64), C.max_err(x32, x64)
    e, m = C.rel_err(got, x64), C.max_err(got, x64)
    print(f"RATIO {what}: rel {e:.3e} = {e / e32:.2f} x E32 ({e32:.2e}), max {m:.3e} = {m / m32:.2f} x ({m32:.2e})")
    assert e <= factor * e32, (what, e, e32, e / e32)
    assert m <= factor * m32, (what, m, m32, m / m32)


def _bank(case, dev):
    B, Fr, H, hop, col0, seed = case
    k = C.bank_case(B, Fr, H, hop, seed, col0)
    d = {n: k[n].to(dev) for n in ("f0_frames", "phase", "g")}
    d["ctrl2d"] = k["ctrl"].reshape(B * Fr, -1).to(dev)
    return k, d


def _bank_forward(ctx, k, d):
    return ctx.sins_bank(d["ctrl2d"], k["col0"], k["H"], d["f0_frames"], d["phase"], k["B"], k["Fr"], k["hop"], SR)


def _bank_adjoint(ctx, k, d):
    """-> (d_ctrl (B*Fr, ld) pre-filled with 7.0, on the host)."""
    d_ctrl = torch.full_like(d["ctrl2d"], 7.0)
    ctx.sins_bank_bwd(d["ctrl2d"], k["col0"], k["H"], d["f0_frames"], d["phase"], d["g"], k["B"], k["Fr"], k["hop"], SR, d_ctrl)
    return d_ctrl.cpu()


def _check_bank_adjoint(what, k, d_ctrl, factor=FACTOR):
    B, Fr, H, col0 = k["B"], k["Fr"], k["H"], k["col0"]
    outside = torch.ones(d_ctrl.shape[1], dtype=torch.bool)
    outside[col0:col0 + H] = False
    assert bool((d_ctrl[:, outside] == 7.0).all()), what          # nothing written beside the block
    got = d_ctrl[:, col0:col0 + H].reshape(B, Fr, H)
    m = k["masked"]
    for name, sel in (("unmasked", ~m), ("masked", m)):
        if sel.any():
            _close(f"{what} adjoint {name}", got[sel], k["d32"][sel], k["d64"][sel], factor)
    _close(f"{what} adjoint all", got, k["d32"], k["d64"], factor)


@pytest.mark.parametrize("case", C.BANK_CASES, ids=C.bank_id)
def test_sins_bank_forward(ctx, dev, case):
    k, d = _bank(case, dev)
    got = _bank_forward(ctx, k, d)
    assert got.shape == (k["B"], k["Fr"] * k["hop"])
    _close(f"bank {C.bank_id(case)} forward", got, k["y32"], k["y64"], CASE_FACTOR.get(("bank", case), FACTOR))
    assert torch.equal(got, _bank_forward(ctx, k, d))


@pytest.mark.parametrize("case", C.BANK_CASES, ids=C.bank_id)
def test_sins_bank_adjoint(ctx, dev, case):
    k, d = _bank(case, dev)
    d_ctrl = _bank_adjoint(ctx, k, d)
    _check_bank_adjoint(f"bank {C.bank_id(case)}", k, d_ctrl, CASE_FACTOR.get(("bank", case), FACTOR))
    assert torch.equal(d_ctrl, _bank_adjoint(ctx, k, d))


def _ola(case, dev):
    B, Fr, seed, comb = case
    k = C.ola_case(B, Fr, seed, comb)
    return k, {n: k[n].to(dev) for n in ("ctrl", "comb", "u", "g")}


@pytest.mark.parametrize("case", C.OLA_CASES, ids=C.ola_id)
def test_spectral_ola_forward(ctx, dev, case):
    import hipddsp
    k, d = _ola(case, dev)
    run = lambda: ctx.spectral_ola(d["ctrl"], d["comb"], d["u"], hipddsp.EXC_UNIT_NOISE, 0, k["B"], k["Fr"], C.OLA_HOP)
    got = run()
    assert got.shape == (k["B"], k["Fr"] * C.OLA_HOP)
    _close(f"ola {C.ola_id(case)} forward", got, k["y32"], k["y64"], CASE_FACTOR.get(("ola", case), FACTOR))
    assert torch.equal(got, run())


@pytest.mark.parametrize("case", C.OLA_CASES, ids=C.ola_id)
def test_spectral_ola_adjoint(ctx, dev, case):
    import hipddsp
    k, d = _ola(case, dev)
    run = lambda: ctx.spectral_ola_bwd(d["ctrl"], d["comb"], d["u"], hipddsp.EXC_UNIT_NOISE, 0, d["g"], k["B"], k["Fr"],
                                       C.OLA_HOP)[:, :3 * C.NB]      # the binding returns empty_like: the rest is undefined
    got = run()
    factor = CASE_FACTOR.get(("ola", case), FACTOR)
    _close(f"ola {C.ola_id(case)} adjoint all", got, k["d32"], k["d64"], factor)
    for name, s in C.OLA_BLOCKS.items():
        _close(f"ola {C.ola_id(case)} adjoint {name}", got[:, s], k["d32"][:, s], k["d64"][:, s], factor)
    assert torch.equal(got, run())


def test_generators_are_pinned(ctx, dev):
    """The draw of each in-kernel generator, bit for bit: EXC_GENERATE with a seed equals EXC_UNIT_NOISE with the host
    restatement of that generator's u (tests/dsp_stage_cases.py).  B = 2 and the seeds 5, 5 + 2**32: the b*T + t index and the
    high seed word both count.  The two generators stay two (`ddsp_hash32` for the FIR and the ragged draw, the splitmix64
    finaliser for the OLA): bench.py outputs depend on each."""
    import hipddsp
    GEN, UNIT = hipddsp.EXC_GENERATE, hipddsp.EXC_UNIT_NOISE
    B, Fr, hop = 2, 2, C.OLA_HOP
    T = Fr * hop
    k, d = _ola((B, Fr, 22, "uniform"), dev)
    rng = np.random.Generator(np.random.PCG64(31))
    ir = torch.from_numpy((rng.standard_normal((B, Fr, 64)) / 8).astype(np.float32)).to(dev)
    outs = []
    for seed in (5, 5 + 2 ** 32):
        u_ola = torch.from_numpy(C.unit_noise_ola(seed, B, T)).to(dev)
        u_fir = torch.from_numpy(C.unit_noise_fir(seed, B, T)).to(dev)
        assert not torch.equal(u_ola, u_fir)
        # spectral OLA, forward and backward
        a = ctx.spectral_ola(d["ctrl"], d["comb"], None, GEN, seed, B, Fr, hop)
        assert torch.equal(a, ctx.spectral_ola(d["ctrl"], d["comb"], u_ola, UNIT, 0, B, Fr, hop))
        assert not torch.equal(a, ctx.spectral_ola(d["ctrl"], d["comb"], u_fir, UNIT, 0, B, Fr, hop))
        ga = ctx.spectral_ola_bwd(d["ctrl"], d["comb"], None, GEN, seed, d["g"], B, Fr, hop)[:, :3 * C.NB]
        gb = ctx.spectral_ola_bwd(d["ctrl"], d["comb"], u_ola, UNIT, 0, d["g"], B, Fr, hop)[:, :3 * C.NB]
        assert torch.equal(ga, gb)
        # LTV-FIR, both arithmetics
        for math in (hipddsp.FIR_FP32, hipddsp.FIR_SPLIT_BF16):
            f, _ = ctx.ltv_fir(None, ir, B, Fr, hop, excitation=GEN, noise_seed=seed, math=math)
            w, _ = ctx.ltv_fir(u_fir, ir, B, Fr, hop, excitation=UNIT, math=math)
            assert torch.equal(f, w), math
            x, _ = ctx.ltv_fir(u_ola, ir, B, Fr, hop, excitation=UNIT, math=math)
            assert not torch.equal(f, x), math
        # the ragged draw with full-length rows is the FIR generator's u itself
        r = ctx.ragged_noise(None, seed, ctx.ragged_counts([Fr] * B), B, Fr, hop)
        assert torch.equal(r, u_fir)
        outs.append((a, f, r))
    for x, y in zip(*outs):
        assert not torch.equal(x, y)


def test_sins_model_with_generic_bank(dev, lib_path):
    """Sins(n_harmonics=100): the forward takes the packed branch, training the generic backward (100 % 32 != 0).  Forward at
    the waveform gate of tests/test_gpu_models.py, gradients with infer=True at the bounds of test_gradients_exact_phase.
    Every block width is a multiple of 4 (100 | 256 | 256)."""
    from ddsp.loss import RSSLoss
    from ddsp.vocoder import Sins
    from conftest import rms
    from oracle import synth as OS
    from test_gpu_training import _oracle_step, _rel
    import synthetic
    cfg = dict(type="Sins", sampling_rate=SR, block_size=512, n_harmonics=100, n_mag_allpass=256, n_mag_noise=256, n_unit=256,
               n_spk=100)
    state = torch.random.get_rng_state()
    torch.manual_seed(13)
    try:
        model = Sins(SR, 512, 100, 256, 256, 256, 100).eval()
    finally:
        torch.random.set_rng_state(state)
    B, Fr = 2, 12
    inp = synthetic.make_inputs(4200, B, Fr)
    sd = model.state_dict()
    with torch.no_grad():
        want = OS.sins_forward(sd, cfg, inp["units"], inp["f0"], inp["volume"], inp["spk_id"], noise=inp["noise"])[0]
    rng = np.random.Generator(np.random.PCG64(10))
    target = torch.from_numpy((0.1 * rng.standard_normal((B, Fr * 512))).astype(np.float32))
    scales = [300, 777, 1531, 2047]
    loss_o, grads_o, _ = _oracle_step(sd, cfg, inp, target, scales, infer=True, kind="Sins")
    model = model.to(dev)
    d = {n: v.to(dev) for n, v in inp.items()}
    with torch.no_grad():
        got = model(d["units"], d["f0"], d["volume"], d["spk_id"], noise=d["noise"])[0]
    assert got.shape == (B, Fr * 512)
    err = rms(got.cpu() - want)
    print("RATIO sins100 forward rms", err)
    assert err < 1e-4, err
    model.train()
    crit = RSSLoss(256, 2048, 4, device=dev)
    sig = model(d["units"], d["f0"], d["volume"], d["spk_id"], infer=True, noise=d["noise"])[0]
    crit.set_scales(scales)
    loss = crit(sig, target.to(dev))
    loss.backward()
    assert abs(float(loss.detach()) - loss_o) < 5e-5 * abs(loss_o)
    errs = sorted(((_rel(p.grad.cpu(), grads_o[n]), n) for n, p in model.named_parameters()), reverse=True)
    print("RATIO sins100 gradients worst", errs[0], "mean", sum(e for e, _ in errs) / len(errs))
    assert errs[0][0] < 2e-2, errs[:5]
    assert sum(e for e, _ in errs) / len(errs) < 5e-3, errs[:5]


def test_sins_bank_bwd_lds_range(ctx, dev):
    """The generic backward keeps 32 * H bytes of sums in dynamic LDS: 64 KiB, the most a launch gets unasked, at H = 2048.
    `ddsp_sins_bank_bwd` refuses more on that path (include/ddsp_amd.h) and launches nothing; partial32 uses no dynamic LDS and
    keeps the forward's range, 4096.  H = 2048 at hop 512 (partial32) against float64 by the module's rule."""
    B, Fr, H, hop, seed = C.LDS_RANGE_CASE
    k = C.bank_case(B, Fr, H, hop, seed)
    d = {n: k[n].to(dev) for n in ("f0_frames", "phase", "g")}
    d["ctrl2d"] = k["ctrl"].reshape(B * Fr, -1).to(dev)
    _close("bank H2048 forward", _bank_forward(ctx, k, d), k["y32"], k["y64"])
    _check_bank_adjoint("bank H2048", k, _bank_adjoint(ctx, k, d))
    # refused: 2049 harmonics at hop 512 (2049 % 32 != 0) and 2080 at hop 1024 are the generic kernel's
    for H_bad, hop_bad in ((2049, 512), (2080, 1024)):
        ctrl = torch.zeros(1, H_bad, device=dev)
        d_ctrl = torch.full_like(ctrl, 7.0)
        z = torch.zeros(1, hop_bad, device=dev)
        with pytest.raises(ValueError):
            ctx.sins_bank_bwd(ctrl, 0, H_bad, torch.full((1, 1, 1), 100.0, device=dev), z, z, 1, 1, hop_bad, SR, d_ctrl)
        assert bool((d_ctrl == 7.0).all())
    # 2080 = 65 * 32 at hop 512 is partial32's: accepted
    ctrl = torch.zeros(1, 2080, device=dev)
    d_ctrl = torch.full_like(ctrl, 7.0)
    z = torch.zeros(1, 512, device=dev)
    ctx.sins_bank_bwd(ctrl, 0, 2080, torch.full((1, 1, 1), 100.0, device=dev), z, z, 1, 1, 512, SR, d_ctrl)
    assert bool((d_ctrl == 0.0).all())                            # a zero upstream gradient
