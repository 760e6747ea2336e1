"""Generates tests/golden/ref_framemix.npz by running the REFERENCE's three synthesisers in this container, on the CPU, with a
`spk_mix_dict` whose values are TENSORS of shape (B, Frame, 1): a speaker mix that changes from frame to frame, which the
reference's `x = x + v * self.spk_embed(id - 1)` broadcasts.

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_framemix.py
The case is tests/framemix_cases.py's: B = 3, Fr = 37, n_spk = 8, ids (2, 5, 8), weights ramping 1 -> 0 / 0 -> 1 / a sine.
What the reference is handed:
  weights  `synthetic.build_model(name, seed, n_spk=8)` (the product's seeded constructor) loaded into the reference's class
           with `load_state_dict(strict=True)` - no second copy is stored, the seed is;
  inputs   `synthetic.make_inputs(seed, 3, 37, n_spk=8)`, its noise injected in place of `torch.rand_like`;
  the mix  {id: torch.from_numpy(weights()[:, :, k : k + 1])} in slot order.
Stand-ins for what the image lacks are make_golden.py's (`_placeholders`).  Recorded: the seeds, the ids, the weight tensor
(B, Fr, K) and, per model, the control matrix (the reference's own sub-module's output, hooked) and the signal - both strided
as framemix_cases says - and their full-length RMS.  Data only."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import framemix_cases as FC  # noqa: E402
import make_golden as MG  # noqa: E402


def main():
    import warnings
    warnings.simplefilter("ignore")
    MG._placeholders()
    import synthetic
    seed_w, seed_in = synthetic.BASE_SEED + 21, synthetic.BASE_SEED + 22
    prod = {}
    for name in FC.NAMES:
        m, cfg = synthetic.build_model(name, seed=seed_w, n_spk=FC.N_SPK)
        prod[name] = ({k: v.clone() for k, v in m.state_dict().items()}, cfg)
    inp = synthetic.make_inputs(seed_in, FC.B, FC.FR, n_spk=FC.N_SPK)
    w = FC.weights()
    mix = {i: torch.from_numpy(w[:, :, k:k + 1].copy()) for k, i in enumerate(FC.IDS)}

    MG._fresh_reference()
    import ddsp.vocoder as V
    assert V.__file__.startswith(MG.REF)
    sys.path.remove(MG.REF)

    g = {"seed_weights": seed_w, "seed_inputs": seed_in, "ids": np.array(FC.IDS, dtype=np.int32), "w": w,
         "signal_step": FC.SIGNAL_STEP, "ctrl_step": FC.CTRL_STEP}
    for name in FC.NAMES:
        sd, cfg = prod[name]
        if name == "CombSub":
            ref = V.CombSub(MG.SR, MG.HOP, cfg["n_mag_allpass"], cfg["n_mag_harmonic"], cfg["n_mag_noise"], 256, cfg["n_spk"])
        elif name == "Sins":
            ref = V.Sins(MG.SR, MG.HOP, cfg["n_harmonics"], cfg["n_mag_allpass"], cfg["n_mag_noise"], 256, cfg["n_spk"])
        else:
            ref = V.CombSubFast(MG.SR, MG.HOP, 256, cfg["n_spk"])
        ref.load_state_dict(sd, strict=True)
        ref.eval()
        grabbed = {}
        h = ref.unit2ctrl.register_forward_hook(lambda m, i, o: grabbed.update(o))
        with torch.no_grad(), MG._InjectNoise(inp["noise"]):
            sig = ref(inp["units"], inp["f0"], inp["volume"], inp["spk_id"], spk_mix_dict=mix)[0]
        h.remove()
        ctrl = torch.cat(list(grabbed.values()), dim=-1)
        assert sig.shape == (FC.B, FC.FR * MG.HOP) and ctrl.shape[:2] == (FC.B, FC.FR)
        assert torch.isfinite(sig).all() and torch.isfinite(ctrl).all()
        g[f"ctrl_{name}"] = ctrl[..., ::FC.CTRL_STEP].contiguous()
        g[f"signal_{name}"] = sig[:, ::FC.SIGNAL_STEP].contiguous()
        g[f"ctrl_rms_{name}"] = float(ctrl.double().pow(2).mean().sqrt())
        g[f"signal_rms_{name}"] = float(sig.double().pow(2).mean().sqrt())
        print(name, "ctrl", tuple(ctrl.shape), "rms", g[f"ctrl_rms_{name}"], "signal rms", g[f"signal_rms_{name}"])
    MG.save("ref_framemix.npz", **g)


if __name__ == "__main__":
    main()
