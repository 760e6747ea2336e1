"""Generates tests/golden/ref_hubert_soft.npz by running the REFERENCE's `encoder/hubert/model.py` `HubertSoft` (and the
tail of its `Units_Encoder.encode`) on the deterministic weight fill of tests/hubert_cases.py, in fp32 and in fp64.

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hubert.py
Stored (fp64 results rounded to fp32, which moves them by ~3e-8 relative):
  keys / shapes / checksums  the state-dict key list, shapes and per-tensor (sum, sum of squares) of the fill
  frames                     conv-stack frame counts of hubert_cases.FRAME_LENGTHS (-1 where the reference raises)
  units64_<case>             HubertSoft.units in fp64 for every case; err32_<case> the reference's own fp32 error (rel. RMS)
  conv64 / pre64 / layer0_64 the "short" case's conv-stack output (B, Fr, 512), the hidden state after the pre-transformer
                             LayerNorm, and after transformer layer 0 (fp64)
  encode32                   Units_Encoder.encode(short audio, 16000, hubert_cases.ENCODE_HOP) with the fp32 model"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from make_golden import REF, _placeholders, save  # noqa: E402
import hubert_cases as HC  # noqa: E402


def rel(a, b):
    return float(((a.double() - b.double()) ** 2).mean().sqrt() / (b.double() ** 2).mean().sqrt())


def main():
    import warnings
    warnings.simplefilter("ignore")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    _placeholders()
    for k in [k for k in sys.modules if k == "ddsp" or k.startswith("ddsp.") or k.startswith("encoder")]:
        del sys.modules[k]
    sys.path.insert(0, REF)
    from encoder.hubert.model import HubertSoft
    import ddsp.vocoder as RV
    sys.path.remove(REF)

    m32 = HubertSoft().eval()
    shapes = {k: tuple(v.shape) for k, v in m32.state_dict().items()}
    sd = HC.fill(shapes)
    m32.load_state_dict(sd, strict=True)
    out = {"keys": np.array(list(shapes)), "shapes": np.array([str(s) for s in shapes.values()]),
           "checksums": HC.checksums(sd)}
    frames = []
    with torch.inference_mode():
        for T in HC.FRAME_LENGTHS:
            try:
                frames.append(m32.feature_extractor(F.pad(torch.zeros(1, 1, T), (40, 40))).shape[-1])
            except RuntimeError:
                frames.append(-1)
    out["frames"] = np.array(frames)
    m64 = HubertSoft().eval()
    m64.load_state_dict(sd, strict=True)
    m64 = m64.double()
    for name in HC.CASES:
        x = HC.audio(name).unsqueeze(1)
        u32 = m32.units(x)
        u64 = m64.units(x.double())
        out[f"units64_{name}"] = u64.float()
        out[f"err32_{name}"] = rel(u32, u64)
        print(name, tuple(u64.shape), "fp32 vs fp64 rel rms", out[f"err32_{name}"], flush=True)
    with torch.inference_mode():
        xp = F.pad(HC.audio("short").unsqueeze(1).double(), (40, 40))
        out["conv64"] = m64.feature_extractor(xp).transpose(1, 2).float()
        out["pre64"] = m64.encode(xp, layer=0)[0].float()
        out["layer0_64"] = m64.encode(xp, layer=1)[0].float()
    enc = object.__new__(RV.Units_Encoder)
    enc.device = "cpu"
    enc.model = lambda a: m32.units(a.unsqueeze(1))
    enc.resample_kernel = {}
    enc.encoder_sample_rate, enc.encoder_hop_size = 16000, 320
    with torch.inference_mode():
        out["encode32"] = enc.encode(HC.audio("short"), 16000, HC.ENCODE_HOP)
    save("ref_hubert_soft.npz", **out)


if __name__ == "__main__":
    main()
