"""`infer_offline.convert`: the offline caller from the raw audio (main.py:88-174 as intended) against `render` fed features
the test extracts itself, and the key shift reaching the model exactly once."""
import numpy as np
import pytest
import torch

import crepe_cases as CC
import hubert_cases as HC
import synthetic

pytestmark = pytest.mark.gpu
SR, HOP = 44100, 512
# (start_sample, end_sample): from 0; after a gap (silence is inserted); overlapping the previous one (cross-fade)
SLICES = [(0, 40000), (45000, 90000), (88000, 132300)]


def _audio():
    """3 s at 44.1 kHz in the style of crepe_cases.audio: a two-octave sweep with a second harmonic and noise."""
    rng = np.random.default_rng(31)
    t = np.arange(3 * SR) / SR
    f = 110.0 * np.exp(np.log(4.0) * t / t[-1])
    ph = 2 * np.pi * np.cumsum(f) / SR
    return (0.3 * np.sin(ph) + 0.15 * np.sin(2 * ph + 0.3) + 0.02 * rng.standard_normal(len(t))).astype(np.float32)


@pytest.fixture(scope="module")
def front(dev, lib_path, tmp_path_factory):
    from ddsp.crepe import Crepe
    from ddsp.hubert import HubertSoft
    from ddsp.vocoder import F0_Extractor, Units_Encoder
    m = Crepe("tiny")
    m.load_state_dict(CC.fill("tiny"))
    path = str(tmp_path_factory.mktemp("hubert") / "hubert-soft.pt")
    torch.save(HC.fill({k: tuple(v.shape) for k, v in HubertSoft().state_dict().items()}), path)
    return Units_Encoder("hubertsoft", path, device=dev), F0_Extractor("crepe", SR, HOP, 65.0, 800.0, crepe_ckpt=m, device=dev)


class _Recording(torch.nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model, self.f0s = model, []

    def forward(self, units, f0, volume, spk_id=None, spk_mix_dict=None, **kw):
        self.f0s.append(f0.clone())
        return self.model(units, f0, volume, spk_id=spk_id, spk_mix_dict=spk_mix_dict, **kw)


@pytest.mark.parametrize("key", [0, 12])
def test_convert_equals_render_on_own_features(dev, front, key):
    """Three slices (from 0; after a gap: silence is inserted; overlapping the previous one: `cross_fade` runs): `convert`
    gives the float64 samples of `render` fed the f0, volume and per-slice units extracted here (main.py:95-110,143-154).
    The extractor dithers by default with a seed from torch's generator: the same generator state gives the same track."""
    import hipddsp
    import infer_offline
    from ddsp.vocoder import DotDict
    encoder, extractor = front
    model, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    spk = torch.full((1, 1), 2, dtype=torch.int64, device=dev)
    audio = _audio()
    torch.manual_seed(17)
    got, sr_o = infer_offline.convert(model, args, audio, SR, SLICES, encoder, extractor, spk, key=key, noise_seed=5)
    x = torch.from_numpy(audio).to(dev)
    torch.manual_seed(17)
    f0 = extractor.extract(x, uv_interp=True)[None, :, None] * 2 ** (key / 12)
    volume = hipddsp.context_for(dev).volume_extract(x[None], HOP)
    segments = [(a // HOP, encoder.encode(x[None, a // HOP * HOP:b // HOP * HOP], SR, HOP)) for a, b in SLICES]
    assert [(s, u.shape[1]) for s, u in segments] == [(0, 79), (87, 89), (171, 88)] and f0.shape[1] == 259
    want, sr_w = infer_offline.render(model, args, segments, f0, volume, spk, noise_seed=5)
    assert sr_o == sr_w == SR and got.dtype == np.float64 and got.shape == want.shape == ((171 + 88) * HOP,)
    assert np.array_equal(got, want)
    assert float(np.abs(got).max()) > 1e-3
    assert np.abs(got[79 * HOP:87 * HOP]).max() == 0.0          # the gap between slices 1 and 2


def test_convert_doubles_f0_exactly_once(dev, front):
    import infer_offline
    from ddsp.vocoder import DotDict
    encoder, extractor = front
    model, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    spk = torch.full((1, 1), 2, dtype=torch.int64, device=dev)
    audio = torch.from_numpy(_audio()).to(dev)
    seen = {}
    for key in (0, 12):
        rec = _Recording(model)
        torch.manual_seed(23)                                   # the same dither draw for both keys
        infer_offline.convert(rec, args, audio, SR, SLICES, encoder, extractor, spk, key=key, noise_seed=5)
        seen[key] = rec.f0s
    assert len(seen[0]) == len(seen[12]) == 3
    for a, b in zip(seen[0], seen[12]):
        assert torch.equal(b, a * 2.0) and float(a.min()) >= 65.0


def test_convert_refuses_a_mismatched_extractor(dev, front):
    import infer_offline
    from ddsp.vocoder import DotDict
    encoder, extractor = front
    model, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    spk = torch.ones(1, 1, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        infer_offline.convert(model, args, _audio(), 48000, SLICES, encoder, extractor, spk)
