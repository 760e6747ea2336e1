"""Generates tests/golden/hop_fir_128.npz, hop_fir_256.npz, hop_ola.npz and hop_models.npz by running the REFERENCE
(/root/reference) on the CPU at block sizes 128 and 256, on the cases of tests/hop_cases.py.

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hop.py

hop_fir_*.npz   the reference's `ddsp/core.py::_fft_convolve` (what `frequency_filter` does with injected filters): the
                output y, and torch autograd's gradients of (y * g).sum() w.r.t. the audio and the filters
hop_ola.npz     the DSP stage of the reference's `CombSubFast.forward` with injected comb (torch.sinc patched for the call),
                noise (torch.rand_like patched) and control (the control network replaced by a stand-in that returns the
                three blocks): output and control gradient in float32 and, from the same code on float64 inputs, float64
hop_models.npz  the reference's three synthesisers (placeholders of make_golden.py for the packages that are not
                installed) with the product's seeded state dict: waveforms for infer = True / False, and one training-mode
                loss and its per-parameter gradient norms (reference RSSLoss, Spectrogram placeholder of make_golden.py,
                scales pinned by patching torch.randint for the call)
The inputs are regenerated from the seeds of tests/hop_cases.py by the tests; only the reference's results are stored."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
import make_golden as MG          # noqa: E402  (also puts the product package on sys.path)
import hop_cases as H             # noqa: E402

REF = MG.REF


def _drop_ddsp():
    for k in [k for k in sys.modules if k == "ddsp" or k.startswith("ddsp.")]:
        del sys.modules[k]


def fir():
    _drop_ddsp()
    sys.path.insert(0, REF)
    import ddsp.core as C
    sys.path.remove(REF)
    assert C.__file__.startswith(REF)
    out = {hop: {} for hop in H.HOPS}
    for case in H.FIR_CASES:
        x, ir, g, _ = H.fir_inputs(case)
        x.requires_grad_(True)
        ir.requires_grad_(True)
        y = C._fft_convolve(x, ir)
        assert y.shape == x.shape
        (y * g).sum().backward()
        y64 = C._fft_convolve(x.detach().double(), ir.detach().double())
        print(H.fir_id(case), "reference fp32 vs its fp64 run: rms %.2e max %.2e" % (
            float((y.detach().double() - y64).pow(2).mean().sqrt()), float((y.detach().double() - y64).abs().max())))
        g_ = out[case[0]]
        g_[H.fir_key(case, "y")] = y.detach()
        g_[H.fir_key(case, "dx")] = x.grad
        g_[H.fir_key(case, "dir")] = ir.grad
    for hop in H.HOPS:
        MG.save(f"hop_fir_{hop}.npz", **out[hop])


class _Patch:
    def __init__(self, name, fn):
        self.name, self.fn = name, fn

    def __enter__(self):
        self.orig = getattr(torch, self.name)
        setattr(torch, self.name, self.fn)

    def __exit__(self, *exc):
        setattr(torch, self.name, self.orig)


def _reference_vocoder():
    warnings.simplefilter("ignore")
    MG._placeholders()
    _drop_ddsp()
    sys.path.insert(0, REF)
    import ddsp.vocoder as V
    sys.path.remove(REF)
    assert V.__file__.startswith(REF)
    return V


def ola(V):
    out = {}
    for case in H.OLA_CASES:
        hop, Fr = case
        nb = hop + 1
        ctrl, comb, u, g = H.ola_inputs(case)
        for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
            ref = V.CombSubFast(H.SR, hop, 4, 1).to(dtype)
            c = ctrl[:, :3 * nb].to(dtype).clone().requires_grad_(True)
            blocks = {n: c[:, i * nb:(i + 1) * nb].reshape(H.B, Fr, nb)
                      for i, n in enumerate(("harmonic_magnitude", "harmonic_phase", "noise_magnitude"))}
            del ref.unit2ctrl
            ref.__dict__["unit2ctrl"] = lambda *a, **k: blocks           # a plain attribute in the sub-module's place
            f0_frames = torch.full((H.B, Fr, 1), 220.0, dtype=dtype)      # voiced everywhere: the injected comb stays as it is
            with _Patch("sinc", lambda x: comb.to(dtype).clone()), _Patch("rand_like", lambda x, *a, **k: u.to(x)):
                y = ref(None, f0_frames, None, None)[0]
            (y * g.to(dtype)).sum().backward()
            out[H.ola_key(case, "y" + tag)] = y.detach()
            out[H.ola_key(case, "d" + tag)] = c.grad.detach()
    MG.save("hop_ola.npz", **out)


def models(V):
    MG._spectrogram_placeholder()
    import ddsp.loss as RL
    assert RL.__file__.startswith(REF)
    prod = {}
    mods = {k: sys.modules.pop(k) for k in [k for k in sys.modules if k == "ddsp" or k.startswith("ddsp.")]}
    for hop in H.HOPS:
        for name in H.MODELS:
            prod[name, hop] = {k: v.clone() for k, v in H.build_model(name, hop).state_dict().items()}
    _drop_ddsp()
    sys.modules.update(mods)
    out = {}
    for hop in H.HOPS:
        inp = H.model_inputs(hop)
        target = H.train_target(hop)
        for name in H.MODELS:
            kw = H.MODEL_KW[name]
            if name == "CombSub":
                ref = V.CombSub(H.SR, hop, kw["n_mag_allpass"], kw["n_mag_harmonic"], kw["n_mag_noise"], H.N_UNIT, H.N_SPK)
            elif name == "Sins":
                ref = V.Sins(H.SR, hop, kw["n_harmonics"], kw["n_mag_allpass"], kw["n_mag_noise"], H.N_UNIT, H.N_SPK)
            else:
                ref = V.CombSubFast(H.SR, hop, H.N_UNIT, H.N_SPK)
            ref.load_state_dict(prod[name, hop], strict=True)
            ref.eval()
            for tag, infer in (("infer", True), ("train", False)):
                with torch.no_grad(), MG._InjectNoise(inp["noise"]):
                    sig, _, (hm, nz) = ref(inp["units"], inp["f0"], inp["volume"], inp["spk_id"], infer=infer)
                out[H.model_key(name, hop, "signal_" + tag)] = sig
                if name != "CombSubFast":
                    out[H.model_key(name, hop, "harmonic_" + tag)] = hm
                    out[H.model_key(name, hop, "noise_" + tag)] = nz
            # one training-mode step's loss and gradients (solver.py:110-113 without the optimiser)
            ref.train()
            crit = RL.RSSLoss(*H.LOSS_RANGE, device="cpu")
            with MG._InjectNoise(inp["noise"]), _Patch("randint", lambda *a, **k: torch.tensor(H.LOSS_SCALES)):
                sig = ref(inp["units"], inp["f0"], inp["volume"], inp["spk_id"], infer=False)[0]
                loss = crit(sig, target)
            loss.backward()
            out[H.model_key(name, hop, "loss")] = loss.detach()
            out[H.model_key(name, hop, "param_names")] = np.array([n for n, _ in ref.named_parameters()])
            out[H.model_key(name, hop, "gradnorm")] = np.array([float(p.grad.norm()) for _, p in ref.named_parameters()])
    MG.save("hop_models.npz", **out)


if __name__ == "__main__":
    torch.set_num_threads(4)
    which = sys.argv[1:] or ["fir", "ola", "models"]
    if "fir" in which:
        fir()
    if "ola" in which or "models" in which:
        V = _reference_vocoder()
        if "ola" in which:
            ola(V)
        if "models" in which:
            models(V)
