"""Generates tests/golden/ragged_models.npz by running the REFERENCE (/root/reference) in this container.

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ragged.py
Same recipe as make_golden.py tier B (its placeholder modules, the product's seeded weights loaded into the reference's
classes, the noise draw injected through torch.rand_like): the reference's own `CombSub / Sins / CombSubFast.forward`
(infer=True) on four utterances of 12, 5, 1 and 9 frames, EACH ALONE at its own length.  The inputs are the rows of one
synthetic batch cut to those lengths, so a test can put them back into one padded batch and render it with `n_frames=`.
The reference tree never travels to the GPU box; only the .npz and this script are committed.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
import make_golden as MG  # noqa: E402  (puts the product package on sys.path)

LENGTHS = [12, 5, 1, 9]
SEED_WEIGHTS_OFFSET, SEED_INPUTS_OFFSET = 7, 23


def main():
    import warnings
    warnings.simplefilter("ignore")
    MG._placeholders()
    for k in [k for k in sys.modules if k == "ddsp" or k.startswith("ddsp.")]:
        del sys.modules[k]
    import synthetic
    prod = {}
    for name in ("CombSub", "Sins", "CombSubFast"):
        m, cfg = synthetic.build_model(name, seed=synthetic.BASE_SEED + SEED_WEIGHTS_OFFSET)
        prod[name] = ({k: v.clone() for k, v in m.state_dict().items()}, cfg)
    for k in [k for k in sys.modules if k == "ddsp" or k.startswith("ddsp.")]:
        del sys.modules[k]
    sys.path.insert(0, MG.REF)
    import ddsp.vocoder as V   # the reference module
    sys.path.remove(MG.REF)
    assert V.__file__.startswith(MG.REF)

    SR, HOP = MG.SR, MG.HOP
    Fr = max(LENGTHS)
    inp = synthetic.make_inputs(synthetic.BASE_SEED + SEED_INPUTS_OFFSET, len(LENGTHS), Fr)
    g = {"seed_weights": synthetic.BASE_SEED + SEED_WEIGHTS_OFFSET, "seed_inputs": synthetic.BASE_SEED + SEED_INPUTS_OFFSET,
         "lengths": np.array(LENGTHS)}
    for name in ("CombSub", "Sins", "CombSubFast"):
        sd, cfg = prod[name]
        if name == "CombSub":
            ref = V.CombSub(SR, HOP, cfg["n_mag_allpass"], cfg["n_mag_harmonic"], cfg["n_mag_noise"], 256, cfg["n_spk"])
        elif name == "Sins":
            ref = V.Sins(SR, HOP, cfg["n_harmonics"], cfg["n_mag_allpass"], cfg["n_mag_noise"], 256, cfg["n_spk"])
        else:
            ref = V.CombSubFast(SR, HOP, 256, cfg["n_spk"])
        ref.load_state_dict(sd, strict=True)
        ref.eval()
        for b, n in enumerate(LENGTHS):
            noise = inp["noise"][b:b + 1, :n * HOP]
            with torch.no_grad(), MG._InjectNoise(noise):
                sig, ph, (hm, nz) = ref(inp["units"][b:b + 1, :n], inp["f0"][b:b + 1, :n], inp["volume"][b:b + 1, :n],
                                        inp["spk_id"][b:b + 1], infer=True)
            g[f"{name}_signal_{b}"] = sig[0]
            g[f"{name}_phase_{b}"] = (ph if ph.shape[1] == n else ph[:, ::HOP])[0, :, 0]
            if name != "CombSubFast":
                g[f"{name}_harmonic_{b}"] = hm[0]
                g[f"{name}_noise_{b}"] = nz[0]
    MG.save("ragged_models.npz", **g)


if __name__ == "__main__":
    main()
