"""`preprocess.analyse_batch` with the real analysers on the device ('tiny' CREPE, the HuBERT fill of tests/hubert_cases.py):
the per-file loop (batch_samples=None) against one ragged group.  Gates: the ragged units test's relative rms per product mode
(tests/test_gpu_hubert.py GATES) and the volume test's 2e-6 relative."""
import numpy as np
import pytest
import torch

import crepe_cases as CC
import hubert_cases as HC
from test_gpu_hubert import GATES

pytestmark = pytest.mark.gpu

SR, HOP = 44100, 512
SECONDS = [0.3, 1.2, 0.55, 0.9]


def _wave(n, f, seed):
    t = np.arange(n) / SR
    rng = np.random.default_rng(seed)
    return (0.3 * np.sin(2 * np.pi * f * t * (1 + 0.2 * t)) + 0.1 * np.sin(4 * np.pi * f * t) + 0.01 * rng.standard_normal(n)).astype(np.float32)


def test_analyse_batch_ragged_group_matches_the_per_file_loop(ctx, dev):
    import hipddsp
    import preprocess as PP
    from ddsp.crepe import Crepe
    from ddsp.vocoder import F0_Extractor, Units_Encoder, Volume_Extractor
    crepe = Crepe("tiny")
    crepe.load_state_dict(CC.fill("tiny"))
    f0x = F0_Extractor("crepe", SR, HOP, 65, 800, crepe_ckpt=crepe, device=dev)
    vol = Volume_Extractor(HOP, device=dev)
    enc = Units_Encoder.__new__(Units_Encoder)       # (the constructor wants a checkpoint file: the fill is loaded instead)
    from ddsp.vocoder import Audio2HubertSoft
    from ddsp.hubert import HubertSoft
    a2h = Audio2HubertSoft.__new__(Audio2HubertSoft)
    torch.nn.Module.__init__(a2h)
    a2h.hubert = HubertSoft()
    a2h.hubert.load_state_dict(HC.fill({k: tuple(v.shape) for k, v in a2h.hubert.state_dict().items()}), strict=True)
    a2h.hubert.to(dev).eval()
    enc.device, enc.model, enc.encoder_sample_rate, enc.encoder_hop_size = dev, a2h.eval(), 16000, 320
    waves = [_wave(int(s * SR) + 7 * i, 130.0 + 50 * i, i) for i, s in enumerate(SECONDS)]
    solo = PP.analyse_batch(waves, f0x, vol, enc, SR, HOP)
    ragged = PP.analyse_batch(waves, f0x, vol, enc, SR, HOP, batch_samples=len(waves) * max(len(w) for w in waves))
    gate = GATES["fp32" if ctx.math == hipddsp.MATH_FP32 else "split"]
    for i, (w, a, b) in enumerate(zip(waves, solo, ragged)):
        n = len(w) // HOP + 1
        for r in (a, b):
            assert r["f0"].shape == (n,) and r["volume"].shape == (n,) and r["units"].shape == (n, 256)
            assert all(isinstance(r[k], np.ndarray) for k in ("f0", "volume", "units"))
            assert np.all(np.isfinite(r["f0"])) and isinstance(r["voiced"], bool)
        assert np.allclose(a["volume"], b["volume"], rtol=2e-6, atol=0), (i, np.abs(a["volume"] - b["volume"]).max())
        rel = float(np.sqrt(np.mean((a["units"].astype(np.float64) - b["units"]) ** 2) / np.mean(b["units"].astype(np.float64) ** 2)))
        print(f"file {i}: units relative rms {rel:.3e} (gate {gate:.0e})")
        assert rel <= gate, (i, rel)
