"""Generates tests/golden/ref_volume_frac.npz by running the REFERENCE's `Volume_Extractor.extract` and the alignment
tail of `Units_Encoder.encode` at non-integral hops (an input at another rate than the model's: main.py:72,109).

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rates.py
The placeholders for absent third-party packages and the path handling are make_golden.py's (tier d does the same at
integral hops); the shapes and seeds are tests/rates_cases.py's."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

from make_golden import REF, _placeholders, save  # noqa: E402
import rates_cases as RC  # noqa: E402


def main():
    import warnings
    warnings.simplefilter("ignore")
    _placeholders()
    for k in [k for k in sys.modules if k == "ddsp" or k.startswith("ddsp.")]:
        del sys.modules[k]
    sys.path.insert(0, REF)
    import ddsp.vocoder as RV
    sys.path.remove(REF)
    out = {}
    for i, h in enumerate(RC.VOLUME_HOPS):
        for j in range(len(RC.volume_lengths(h))):
            audio, hop = RC.volume_audio(i, j)
            out[f"vol_{i}_{j}"] = RV.Volume_Extractor(hop).extract(audio)
    for i in range(len(RC.ALIGN_CASES)):
        units, n = RC.align_input(i)
        enc = object.__new__(RV.Units_Encoder)
        enc.device = "cpu"
        enc.model = lambda a, u=units: u
        enc.resample_kernel = {str(RC.ALIGN_SR): (lambda a: a)}
        enc.encoder_sample_rate, enc.encoder_hop_size = 16000, 320
        out[f"align_{i}"] = enc.encode(torch.zeros(1, n), RC.ALIGN_SR, RC.ALIGN_HOP)
    save("ref_volume_frac.npz", **out)


if __name__ == "__main__":
    main()
