"""Ragged HuBERT-Soft, host side (no GPU): the entry points that take the counts are exported and bound, `n_samples=` is checked before any
device work, `convert_batched` has its new keyword, and the grouping by sample length covers every slice exactly once."""
import inspect

import numpy as np
import pytest
import torch

NEW = ["ddsp_hubert_soft_units", "ddsp_hubert_encode", "ddsp_softmax_attention", "ddsp_resample", "ddsp_align_units"]
T = 8000


class _OnDevice(torch.Tensor):
    """A tensor that reports `is_cuda` (there is no device on this side of the suite)."""
    is_cuda = property(lambda self: True)


def test_new_symbols_are_exported_and_bound(lib_path):
    import hipddsp
    lib = hipddsp.load_library()
    for name in NEW:
        assert name in hipddsp.SIGNATURES, name
        assert getattr(lib, name).argtypes == hipddsp.SIGNATURES[name][1]
    assert hipddsp.ABI_VERSION == 8 and lib.ddsp_abi_version() == 8
    for m in ("hubert_units", "hubert_encode"):
        assert "n_dev" in inspect.signature(getattr(hipddsp.Context, m)).parameters
    # one binding method per operation: the ragged form is an argument of the un-suffixed method
    for m, names in (("softmax_attention", ["n_keys_dev"]), ("resample", ["n_dev"]), ("align_units", ["n_units_dev", "n_out_dev"])):
        for n in names:
            assert inspect.signature(getattr(hipddsp.Context, m)).parameters[n].default is None, (m, n)
    assert not [a for a in dir(hipddsp.Context) if a.endswith("_ragged")]


def _bad_counts():
    """Counts for a (3, T) batch that must be refused: wrong length, 0, > T, too short for the conv stack (319 samples give
    no frame, 320 give one), a device tensor, non-ints, wrong rank."""
    return [[T, T], [T] * 4, [0, T, T], [T, T + 1, T], [T, -5, T], [T, 319, T], torch.tensor([T, 319, T]),
            torch.tensor([T, T, T]).as_subclass(_OnDevice), [float(T), T, T], [True, T, T], T, "888",
            torch.tensor([float(T)] * 3), torch.tensor([[T, T, T]]), torch.tensor([T, T]), np.array([T, T, T + 7])]


def test_bad_n_samples_raise_before_any_device_work(lib_path):
    """CPU tensors: a valid call ends in the 'HIP device only' RuntimeError; a bad n_samples must be refused first."""
    from ddsp.hubert import HubertSoft
    m = HubertSoft().eval()
    wav = torch.zeros(3, 1, T)
    for n in _bad_counts():
        with pytest.raises(ValueError):
            m.units(wav, n_samples=n)
        with pytest.raises(ValueError):
            m.units(wav, n)
        with pytest.raises(ValueError):
            m.encode(wav, layer=-1, n_samples=n)
        with pytest.raises(ValueError):
            m(wav, n_samples=n)
    for n in ([T, 320, 5000], (T, 320, 5000), torch.tensor([T, 320, 5000]), torch.tensor([T, 320, 5000], dtype=torch.int32),
              np.array([T, 320, 5000])):
        with pytest.raises(RuntimeError, match="HIP device"):
            m.units(wav, n_samples=n)
        with pytest.raises(RuntimeError, match="HIP device"):
            m.encode(wav, n_samples=n)
    with pytest.raises(RuntimeError, match="HIP device"):       # None is the rectangular call
        m.units(wav)


def test_signatures():
    import infer_offline
    from ddsp.hubert import HubertSoft
    from ddsp.vocoder import Audio2HubertSoft, Units_Encoder
    p = inspect.signature(infer_offline.convert_batched).parameters
    assert list(p)[-1] == "units_batch_samples" and p["units_batch_samples"].default is None
    assert "units_batch_samples" not in inspect.signature(infer_offline.convert).parameters
    assert list(inspect.signature(HubertSoft.units).parameters) == ["self", "wav", "n_samples"]
    assert list(inspect.signature(HubertSoft.encode).parameters) == ["self", "wav", "layer", "n_samples"]
    assert list(inspect.signature(Audio2HubertSoft.forward).parameters) == ["self", "audio", "n_samples"]
    assert list(inspect.signature(Units_Encoder.encode).parameters) == ["self", "audio", "sample_rate", "hop_size", "n_samples"]
    for f, name in ((HubertSoft.units, "n_samples"), (HubertSoft.encode, "n_samples"), (Audio2HubertSoft.forward, "n_samples"),
                    (Units_Encoder.encode, "n_samples")):
        assert inspect.signature(f).parameters[name].default is None


class _StubEncoder:
    """`Units_Encoder.encode` of a ragged batch with units[b, i, 0] = the first sample of row b; records the calls."""

    def __init__(self):
        self.calls = []

    def encode(self, audio, sample_rate, hop_size, n_samples=None):
        self.calls.append((tuple(audio.shape), list(n_samples)))
        n = [int(v // hop_size) + 1 for v in n_samples]
        out = torch.zeros(audio.shape[0], max(n), 4)
        for b, k in enumerate(n):
            out[b, :k] = audio[b, 0]
        return out


def test_unit_groups_cover_every_slice_once_in_order(lib_path):
    from infer_offline import _encode_ragged, group_segments
    rng = np.random.Generator(np.random.PCG64(5))
    hop = 512 * 44100 / 48000
    for trial in range(20):
        lengths = [int(x) for x in rng.integers(2000, 60000, size=int(rng.integers(1, 12)))]
        budget = int(rng.integers(1, 200000))
        pieces = [(7 * i, torch.full((1, n), float(i + 1))) for i, n in enumerate(lengths)]
        stub = _StubEncoder()
        out = _encode_ragged(stub, pieces, 44100, hop, budget)
        groups = group_segments(lengths, budget)
        assert sorted(i for g in groups for i in g) == list(range(len(lengths)))
        assert len(stub.calls) == len(groups)
        for g, (shape, counts) in zip(groups, stub.calls):
            assert counts == [lengths[i] for i in g] and shape == (len(g), max(counts))
            assert shape[0] * shape[1] <= budget or len(g) == 1
        assert [s for s, _ in out] == [7 * i for i in range(len(lengths))]
        for i, (_, u) in enumerate(out):
            assert u.shape == (1, int(lengths[i] // hop) + 1, 4) and bool((u == float(i + 1)).all())


def test_units_encoder_checks_counts_at_its_own_rate(lib_path, tmp_path):
    """Counts are at `sample_rate`: 880 samples at 44.1 kHz are 320 at 16 kHz (one frame), 879 are 319 (none)."""
    import hipddsp
    from ddsp.vocoder import Units_Encoder
    assert hipddsp.load_library().ddsp_resample_length(880, 44100, 16000) == 320
    enc = Units_Encoder.__new__(Units_Encoder)
    enc.encoder_sample_rate, enc.encoder_hop_size = 16000, 320
    audio = torch.zeros(2, 30000)
    for bad in ([30000], [30000, 30001], [30000, 0], [30000, 879], torch.tensor([30000, 30000]).as_subclass(_OnDevice)):
        with pytest.raises(ValueError):
            enc.encode(audio, 44100, 512, n_samples=bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        enc.encode(audio, 44100, 512, n_samples=[30000, 880])
