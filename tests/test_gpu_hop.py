"""Block sizes 128 and 256: the frame-varying FIR (csrc/ltv_fir_hop.hip), the spectral overlap-add (csrc/spectral_ola.hip at
N = 256 / 512) and the three synthesisers on them, against fixtures the reference computed on the CPU
(tests/golden/make_golden_hop.py; cases and inputs: tests/hop_cases.py).

Every bound is one an existing test applies to the same comparison at 512; the line is cited where it is used."""
import os

import numpy as np
import pytest
import torch

import dsp_stage_cases as SC
import hop_cases as H
from conftest import GOLDEN, rms

pytestmark = pytest.mark.gpu
GATE = 1e-4                      # tests/test_gpu_models.py:18, the waveform gate


@pytest.fixture(scope="module")
def fix():
    z = {}
    for name in ("hop_fir_128.npz", "hop_fir_256.npz", "hop_ola.npz", "hop_models.npz"):
        with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as f:
            z.update({k: f[k] for k in f.files})
    return z


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


# ---- frame-varying FIR ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", H.FIR_CASES, ids=H.fir_id)
def test_fir_forward(ctx, dev, fix, case):
    """Against the reference's `_fft_convolve`; bounds of tests/test_gpu_dsp.py:116-117 (fp32 pipe, signals of that scale)."""
    hop, Fr, n, with_add = case
    x, ir, _, add = H.fir_inputs(case)
    want = _t(fix[H.fir_key(case, "y")]).double()
    got, got_sum = ctx.ltv_fir(x.to(dev), ir.to(dev), H.B, Fr, hop, add_in=add.to(dev) if with_add else None)
    got = got.cpu()
    assert got.shape == (H.B, Fr * hop)
    e, m = rms(got.double() - want), float((got.double() - want).abs().max())
    print(f"FIGURE fir {H.fir_id(case)}: rms {e:.3e} max {m:.3e}")
    assert e < 1e-6
    assert m < 1e-5
    if with_add:
        assert torch.equal(got_sum.cpu(), add + got)          # tests/test_gpu_dsp.py:136
        only_sum = ctx.ltv_fir(x.to(dev), ir.to(dev), H.B, Fr, hop, add_in=add.to(dev), want_out=False)
        assert only_sum[0] is None and torch.equal(only_sum[1].cpu(), add + got)
    else:
        assert got_sum is None
    # the context's product mode does not reach these hops: fp32 products whatever `math` says
    import hipddsp
    again, _ = ctx.ltv_fir(x.to(dev), ir.to(dev), H.B, Fr, hop, math=hipddsp.FIR_SPLIT_BF16)
    assert torch.equal(again.cpu(), got)
    # unit-noise excitation is the audio 2u - 1 (exact in fp32)
    u = _t(SC.unit_noise_fir(3, H.B, Fr * hop))
    a, _ = ctx.ltv_fir(u.to(dev), ir.to(dev), H.B, Fr, hop, excitation=hipddsp.EXC_UNIT_NOISE)
    b_, _ = ctx.ltv_fir((u * 2 - 1).to(dev), ir.to(dev), H.B, Fr, hop)
    assert torch.equal(a, b_)


@pytest.mark.parametrize("hop", H.HOPS)
def test_noise_stream_is_the_one_of_hop_512(ctx, dev, hop):
    """Unit impulses at tap n/2 return the excitation (the two window shares of a sample sum to 1 within an ulp): the generated
    stream of one seed and one (B, T) is the same function of (seed, row, sample) at every hop.  1e-6 absolute on [-1, 1)."""
    import hipddsp
    B, T, n, seed = 2, 2048, 32, 77
    outs = {}
    for h in (hop, 512):
        ir = torch.zeros(B, T // h, n)
        ir[..., n // 2] = 1.0
        outs[h], _ = ctx.ltv_fir(None, ir.to(dev), B, T // h, h, excitation=hipddsp.EXC_GENERATE, noise_seed=seed)
    want = _t(SC.unit_noise_fir(seed, B, T)) * 2 - 1
    assert float((outs[512].cpu() - want).abs().max()) <= 1e-6
    assert float((outs[hop] - outs[512]).abs().max()) <= 1e-6
    assert float(outs[hop].abs().max()) > 0.9


@pytest.mark.parametrize("case", H.FIR_CASES, ids=H.fir_id)
def test_fir_adjoint(ctx, dev, fix, case):
    """d_audio and d_ir against torch autograd through the reference's `_fft_convolve`; bound of
    tests/test_gpu_backward.py:29-30 (relative 2-norm < 2e-5), and either output alone."""
    hop, Fr, n, _ = case
    x, ir, g, _ = H.fir_inputs(case)
    dx, dir_ = ctx.ltv_fir_bwd(x.to(dev), ir.to(dev), g.to(dev), H.B, Fr, hop)
    ex, ei = _rel(dx.cpu(), _t(fix[H.fir_key(case, "dx")])), _rel(dir_.cpu().reshape(H.B, Fr, n), _t(fix[H.fir_key(case, "dir")]))
    print(f"FIGURE fir adjoint {H.fir_id(case)}: d_audio {ex:.3e} d_ir {ei:.3e}")
    assert ex < 2e-5
    assert ei < 2e-5
    only_x = ctx.ltv_fir_bwd(x.to(dev), ir.to(dev), g.to(dev), H.B, Fr, hop, want_d_ir=False)
    only_i = ctx.ltv_fir_bwd(x.to(dev), ir.to(dev), g.to(dev), H.B, Fr, hop, want_d_audio=False)
    assert only_x[1] is None and only_i[0] is None
    assert torch.equal(only_x[0], dx) and torch.equal(only_i[1], dir_)


@pytest.mark.parametrize("hop", H.HOPS)
def test_fir_adjoint_regenerates_the_noise(ctx, dev, hop):
    """d_ir with EXC_GENERATE is d_ir with the same stream injected as unit noise."""
    import hipddsp
    B, Fr, n, seed = 2, 5, 510, 9
    rng = np.random.Generator(np.random.PCG64(hop))
    ir = torch.from_numpy((rng.standard_normal((B, Fr, n)) / np.sqrt(n)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal((B, Fr * hop)).astype(np.float32)).to(dev)
    u = _t(SC.unit_noise_fir(seed, B, Fr * hop)).to(dev)
    _, d_gen = ctx.ltv_fir_bwd(None, ir, g, B, Fr, hop, excitation=hipddsp.EXC_GENERATE, noise_seed=seed, want_d_audio=False)
    _, d_inj = ctx.ltv_fir_bwd(u, ir, g, B, Fr, hop, excitation=hipddsp.EXC_UNIT_NOISE, want_d_audio=False)
    assert torch.equal(d_gen, d_inj) and float(d_gen.abs().max()) > 0


# ---- spectral overlap-add ---------------------------------------------------------------------------------------------
FACTOR = 16.0                    # tests/test_gpu_dsp_stages.py:48


def _close(what, got, x32, x64):
    """The rule of tests/test_gpu_dsp_stages.py:53-61: the device's distance from the float64 reference is at most FACTOR times
    the float32 reference's own, as relative 2-norm and as max-abs."""
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == x64.shape and bool(torch.isfinite(got).all()), what
    e32, m32 = SC.rel_err(x32, x64), SC.max_err(x32, x64)
    e, m = SC.rel_err(got, x64), SC.max_err(got, x64)
    print(f"RATIO {what}: rel {e:.3e} = {e / e32:.2f} x E32 ({e32:.2e}), max {m:.3e} = {m / m32:.2f} x ({m32:.2e})")
    assert e <= FACTOR * e32, (what, e, e32, e / e32)
    assert m <= FACTOR * m32, (what, m, m32, m / m32)


@pytest.mark.parametrize("case", H.OLA_CASES, ids=H.ola_id)
def test_spectral_ola_forward_and_adjoint(ctx, dev, fix, case):
    """Against the DSP stage of the reference's `CombSubFast.forward` with injected comb, noise and control."""
    import hipddsp
    hop, Fr = case
    nb = hop + 1
    ctrl, comb, u, g = (v.to(dev) for v in H.ola_inputs(case))
    y32, y64, d32, d64 = (_t(fix[H.ola_key(case, k)]) for k in ("y32", "y64", "d32", "d64"))
    got = ctx.spectral_ola(ctrl, comb, u, hipddsp.EXC_UNIT_NOISE, 0, H.B, Fr, hop)
    assert got.shape == (H.B, Fr * hop)
    _close(f"ola {H.ola_id(case)} forward", got, y32, y64)
    d = ctx.spectral_ola_bwd(ctrl, comb, u, hipddsp.EXC_UNIT_NOISE, 0, g, H.B, Fr, hop)[:, :3 * nb]
    _close(f"ola {H.ola_id(case)} adjoint all", d, d32, d64)
    for i, name in enumerate(("hm", "hp", "nm")):
        s = slice(i * nb, (i + 1) * nb)
        _close(f"ola {H.ola_id(case)} adjoint {name}", d[:, s], d32[:, s], d64[:, s])
    # the generated excitation is the stream of `noise_u` there, whatever the frame length
    seed = 21
    ug = _t(SC.unit_noise_ola(seed, H.B, Fr * hop)).to(dev)
    assert torch.equal(ctx.spectral_ola(ctrl, comb, None, hipddsp.EXC_GENERATE, seed, H.B, Fr, hop),
                       ctx.spectral_ola(ctrl, comb, ug, hipddsp.EXC_UNIT_NOISE, 0, H.B, Fr, hop))


# ---- models -----------------------------------------------------------------------------------------------------------
def _dev_inputs(hop, dev):
    return {k: v.to(dev) for k, v in H.model_inputs(hop).items()}


@pytest.mark.parametrize("hop", H.HOPS)
@pytest.mark.parametrize("name", H.MODELS)
def test_model_against_reference(dev, lib_path, fix, name, hop):
    """Waveforms of the reference's own forward, `infer` both ways, at the gate of tests/test_gpu_models.py:113-114,180."""
    model = H.build_model(name, hop, dev)
    d = _dev_inputs(hop, dev)
    for tag, infer in (("infer", True), ("train", False)):
        with torch.no_grad():
            sig, ph, (hm, nz) = model(d["units"], d["f0"], d["volume"], d["spk_id"], infer=infer, noise=d["noise"])
        assert sig.shape == (H.B, H.MODEL_FR * hop)
        e = rms(sig.cpu() - _t(fix[H.model_key(name, hop, "signal_" + tag)]))
        print(f"FIGURE model {name} hop {hop} {tag}: rms {e:.3e}")
        assert e < GATE, (name, hop, tag, e)
        if name != "CombSubFast":
            assert rms(hm.cpu() - _t(fix[H.model_key(name, hop, "harmonic_" + tag)])) < GATE
            assert rms(nz.cpu() - _t(fix[H.model_key(name, hop, "noise_" + tag)])) < GATE


@pytest.mark.parametrize("hop", H.HOPS)
@pytest.mark.parametrize("name", H.MODELS)
def test_model_ragged(dev, lib_path, name, hop):
    """n_frames = [9, 4]: each row is its solo render over its own frames (the gate of tests/test_gpu_ragged.py:140) and
    exactly 0 after them (:141)."""
    model = H.build_model(name, hop, dev)
    d = _dev_inputs(hop, dev)
    with torch.no_grad():
        sig = model(d["units"], d["f0"], d["volume"], d["spk_id"], noise=d["noise"], n_frames=H.MODEL_RAGGED)[0]
        assert sig.shape == (H.B, H.MODEL_FR * hop) and bool(torch.isfinite(sig).all())
        for b, n in enumerate(H.MODEL_RAGGED):
            solo = model(d["units"][b:b + 1, :n].contiguous(), d["f0"][b:b + 1, :n].contiguous(),
                         d["volume"][b:b + 1, :n].contiguous(), d["spk_id"][b:b + 1],
                         noise=d["noise"][b:b + 1, :n * hop].contiguous())[0]
            e = rms(sig[b, :n * hop].cpu() - solo[0].cpu())
            print(f"FIGURE ragged {name} hop {hop} row {b}: rms {e:.3e} of {rms(solo.cpu()):.3e}")
            assert e < GATE, (name, hop, b, e)
            assert rms(solo.cpu()) > 1e-3
            assert torch.count_nonzero(sig[b, n * hop:]) == 0


@pytest.mark.parametrize("hop", H.HOPS)
@pytest.mark.parametrize("name", H.MODELS)
def test_model_training_backward(dev, lib_path, fix, name, hop):
    """One training-mode forward, loss and backward: the loss at tests/test_gpu_training.py:198 (2e-4 relative), the
    per-parameter gradient norms at :203 (rtol 5e-2, atol 1e-6) of the reference run."""
    from ddsp.loss import RSSLoss
    model = H.build_model(name, hop, dev).train()
    names = [n for n, _ in model.named_parameters()]
    assert names == [str(n) for n in fix[H.model_key(name, hop, "param_names")]]
    d = _dev_inputs(hop, dev)
    crit = RSSLoss(*H.LOSS_RANGE, device=dev)
    crit.set_scales(H.LOSS_SCALES)
    sig = model(d["units"], d["f0"], d["volume"], d["spk_id"], infer=False, noise=d["noise"])[0]
    loss = crit(sig, H.train_target(hop).to(dev))
    loss.backward()
    want = float(fix[H.model_key(name, hop, "loss")])
    loss = loss.detach()
    assert abs(float(loss) - want) < 2e-4 * want, (float(loss), want)
    gn = np.array([float(p.grad.norm()) for _, p in model.named_parameters()])
    ref = fix[H.model_key(name, hop, "gradnorm")]
    print(f"FIGURE train {name} hop {hop}: loss {float(loss):.6f} / {want:.6f}, worst gradnorm ratio "
          f"{np.abs(gn / np.maximum(ref, 1e-12) - 1)[ref > 1e-6].max():.3e}")
    assert np.allclose(gn, ref, rtol=5e-2, atol=1e-6), np.abs(gn / np.maximum(ref, 1e-12) - 1).max()


# ---- refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [64, 160, 1024])
def test_other_hops_are_refused(ctx, dev, hop):
    import hipddsp
    B, Fr, n = 1, 2, 32
    T = Fr * hop
    x, ir, g = torch.zeros(B, T, device=dev), torch.zeros(B, Fr, n, device=dev), torch.zeros(B, T, device=dev)
    ctrl = torch.zeros(B * Fr, 3 * (hop + 1), device=dev)
    calls = [lambda: ctx.ltv_fir(x, ir, B, Fr, hop),
             lambda: ctx.ltv_fir_bwd(x, ir, g, B, Fr, hop),
             lambda: ctx.spectral_ola(ctrl, x, x, hipddsp.EXC_UNIT_NOISE, 0, B, Fr, hop),
             lambda: ctx.spectral_ola_bwd(ctrl, x, x, hipddsp.EXC_UNIT_NOISE, 0, g, B, Fr, hop)]
    for call in calls:
        with pytest.raises(ValueError, match="128, 256 or 512"):
            call()
