"""CPU-side checks of the base-form units encoder ('cvec', 'cvec768'; `ddsp.hubert.HubertBase`): fairseq's state-dict contract as
tests/golden/ref_hubert_base.npz records it, the checkpoint loader, the no-pad frame rule against the reference's conv stack,
the `Units_Encoder` names, and every refusal that must come before a launch."""
import os
import pickle
import sys
import types

import numpy as np
import pytest
import torch

import hubert_base_cases as BC
import hubert_cases as HC
import synthetic
from conftest import GOLDEN


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLDEN, "ref_hubert_base.npz"))


@pytest.fixture(scope="module")
def fill(fix):
    """(fairseq-named state dict, reference-named state dict) of the deterministic fill."""
    return BC.fairseq_fill(fix, np.load(os.path.join(GOLDEN, "ref_hubert_soft.npz")))


def test_state_dict_keys_and_shapes_are_fairseqs(fix):
    from ddsp.hubert import HubertBase
    own = {k: tuple(v.shape) for k, v in HubertBase().state_dict().items()}
    table = BC.table_of(fix)
    want = {fs: shape for _, fs, shape, _ in table}
    want["label_embs_concat"] = own["label_embs_concat"]          # (its rows differ between checkpoints: any count loads)
    assert list(own) == [fs for _, fs, _, _ in table]
    assert own == want
    assert len(own) == 214 and own["encoder.layers.8.self_attn.k_proj.weight"] == (768, 768)


def test_fill_under_fairseq_names_reproduces_the_fixture_checksums(fix, fill):
    np.testing.assert_allclose(HC.checksums(fill[0]), fix["checksums"], rtol=1e-12, atol=1e-9)


def test_fairseq_state_dict_loads_strict_in_every_wrapping(fill):
    from ddsp.hubert import HubertBase, load_fairseq_state
    sd = fill[0]
    assert sd["label_embs_concat"].shape == (100, 256)            # not HubertBase's own 504 rows
    for obj in (sd, {"model": sd, "cfg": None}, {"module." + k: v for k, v in sd.items()},
                {"model": {"module." + k: v for k, v in sd.items()}}, {**sd, "label_embs_concat": torch.zeros(7, 256)}):
        m = HubertBase()
        got = load_fairseq_state(obj)
        assert list(got) == list(sd)
        res = m.load_state_dict(got, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert torch.equal(m.encoder.layers[3].self_attn.v_proj.weight, sd["encoder.layers.3.self_attn.v_proj.weight"])
        assert m.label_embs_concat.shape == got["label_embs_concat"].shape
    with pytest.raises(ValueError):
        load_fairseq_state({"model": 3})
    with pytest.raises(RuntimeError):                              # a missing tensor is still an error
        HubertBase().load_state_dict({k: v for k, v in sd.items() if k != "final_proj.bias"})


def test_checkpoint_with_fairseq_objects_says_what_to_do(tmp_path, fill):
    """A checkpoint as fairseq's trainer writes it pickles its config classes: without the package the loader must say so."""
    from ddsp.hubert import read_fairseq_checkpoint
    name = "fairseq_standin_for_this_test"
    mod = types.ModuleType(name)
    mod.Cfg = type("Cfg", (), {"__module__": name})
    sys.modules[name] = mod
    try:
        torch.save({"model": {"final_proj.bias": fill[0]["final_proj.bias"]}, "cfg": mod.Cfg()}, str(tmp_path / "trainer.pt"))
    finally:
        del sys.modules[name]
    with pytest.raises(RuntimeError, match=r"fairseq / omegaconf objects(.|\n)*machine that has fairseq(.|\n)*ckpt\['model'\]"):
        read_fairseq_checkpoint(str(tmp_path / "trainer.pt"))
    plain = str(tmp_path / "plain.pt")
    torch.save({"model": fill[0]}, plain)
    assert list(read_fairseq_checkpoint(plain)) == list(fill[0])
    with pytest.raises((pickle.UnpicklingError, RuntimeError, EOFError)):
        open(str(tmp_path / "junk.pt"), "wb").write(b"not a checkpoint")
        read_fairseq_checkpoint(str(tmp_path / "junk.pt"))


def test_frame_rule_matches_the_reference_conv_stack_without_padding(lib_path, fix):
    import hipddsp
    from ddsp.hubert import HubertBase
    lengths = list(HC.FRAME_LENGTHS) + list(BC.EXTRA_FRAME_LENGTHS)
    wants = list(fix["frames0"]) + list(fix["frames0_extra"])
    assert {399, 400, 401, 719, 720} <= set(lengths)
    for T, want in zip(lengths, wants):
        got = hipddsp.hubert_base_frames(T)
        assert got == max(int(want), 0), (T, got, want)
        if want <= 0:
            with pytest.raises(ValueError):
                HubertBase.frames(T)
        else:
            assert HubertBase.frames(T) == want
    by = dict(zip(lengths, wants))
    assert by[399] == -1 and by[400] == 1 and by[401] == 1 and by[719] == 1 and by[720] == 2
    assert hipddsp.hubert_base_frames(-1) == -1
    # the padded rule of HuBERT-Soft is the same rule 80 samples later
    assert all(hipddsp.hubert_frames(T) == hipddsp.hubert_base_frames(T + 80) for T in range(0, 2000, 7))


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory, fill):
    path = str(tmp_path_factory.mktemp("cvec") / "cvec-state.pt")
    torch.save(fill[0], path)
    return path


class _Dev:
    """`Units_Encoder` asks for a HIP device; on a machine without one the host-side tests name it and move nothing there."""

    def __enter__(self):
        from ddsp import hubert
        self._to = hubert.HubertBase.to
        hubert.HubertBase.to = lambda m, *a, **k: m
        return "cuda"

    def __exit__(self, *exc):
        from ddsp import hubert
        hubert.HubertBase.to = self._to


@pytest.mark.parametrize("name,width", [("cvec", 256), ("cvec768", 768)])
def test_units_encoder_constructs_from_a_state_dict_file(lib_path, ckpt, fill, name, width):
    from ddsp.vocoder import Audio2CVec, Audio2CVec768, Units_Encoder
    with _Dev() as dev:
        enc = Units_Encoder(name, ckpt, device=dev)
    assert enc.n_unit == width and enc.encoder == name and not enc.padded
    assert type(enc.model) is (Audio2CVec if width == 256 else Audio2CVec768)
    assert torch.equal(enc.model.hubert.final_proj.weight, fill[0]["final_proj.weight"])
    # the no-pad rule: 400 samples at 16 kHz, and what resamples to them from 44.1 kHz
    import hipddsp
    assert enc.min_samples(16000) == 400
    lo = enc.min_samples(44100)
    assert hipddsp.hubert_base_frames(hipddsp.resample_length(lo, 44100, 16000)) == 1
    assert hipddsp.hubert_base_frames(hipddsp.resample_length(lo - 1, 44100, 16000)) == 0
    soft = Units_Encoder.__new__(Units_Encoder)                    # (the class defaults are HuBERT-Soft's)
    soft.encoder_sample_rate = 16000
    assert soft.min_samples(16000) == 320 and soft.padded and soft.n_unit == 256
    # refusals that come before any launch
    with pytest.raises(ValueError):
        enc.encode(torch.zeros(2, 4000), 16000, 160, n_samples=[4000, 399])     # a row too short under the no-pad rule
    with pytest.raises(ValueError):
        enc.encode(torch.zeros(2, 4000), 16000, 160, n_samples=[4000])
    with pytest.raises(RuntimeError):
        enc.encode(torch.zeros(1, 4000), 16000, 160)                            # a CPU tensor
    with pytest.raises(RuntimeError):
        enc.encode(torch.zeros(2, 4000), 16000, 160, n_samples=[4000, 400])


def test_reference_names_still_raise_and_name_the_new_ones():
    from ddsp.vocoder import Units_Encoder
    for name in ("hubertbase", "hubertbase768", "contentvec", "contentvec768", "xunit", "yunit"):
        with pytest.raises(NotImplementedError, match="hubertsoft") as e:
            Units_Encoder(name, "unused.pt")
        if not name.endswith("unit"):
            assert ("'cvec768'" if name.endswith("768") else "'cvec'") in str(e.value)
    with pytest.raises(ValueError):
        Units_Encoder("cvec512", "unused.pt")


def test_cpu_tensors_and_bad_counts_are_refused_before_any_launch(lib_path):
    from ddsp.hubert import HubertBase
    m = HubertBase()
    with pytest.raises(RuntimeError):
        m.units(torch.zeros(1, 1, 8000))
    with pytest.raises(RuntimeError):
        m.units(torch.zeros(2, 1, 8000), n_samples=[8000, 400])
    for bad in ([8000], [8000, 0], [8000, 8001], [8000, 399], [8000, 5.5], torch.tensor([8000.0, 400.0])):
        with pytest.raises(ValueError):
            m.units(torch.zeros(2, 1, 8000), n_samples=bad)
    for layer in (0, 13):
        with pytest.raises(ValueError):
            m.units(torch.zeros(1, 1, 8000), layer=layer)


def test_width_mismatch_is_a_value_error_at_construction(lib_path, ckpt):
    import infer_offline
    import realtime
    from ddsp.analysis import check_units_width
    from ddsp.vocoder import Units_Encoder
    with _Dev() as dev:
        wide = Units_Encoder("cvec768", ckpt, device=dev)
    m256, _ = synthetic.build_model("CombSubFast", seed=5)
    m768, _ = synthetic.build_model("CombSubFast", seed=5, n_unit=768)
    check_units_width("test", wide, m768)
    with pytest.raises(ValueError, match="768 channels"):
        check_units_width("test", wide, m768, m256)
    with pytest.raises(ValueError, match="768 channels"):
        realtime.StreamRenderer(m256, 44100, 0.2, 0.04, "cpu", use_graph=False, units_encoder=wide, f0_extractor="ac")
    with pytest.raises(ValueError, match="768 channels"):
        realtime.StreamBank(m256, 2, 44100, 0.2, 0.04, "cpu", use_graph=False, units_encoder=wide, f0_extractor="ac")
    with pytest.raises(ValueError, match="768 channels"):
        infer_offline.convert_device(m256, None, torch.zeros(44100), 44100, None, wide, None, 1)
    with pytest.raises(ValueError, match="768 channels"):
        infer_offline.convert_many_device(m256, None, [torch.zeros(44100)], 44100, wide, None, spk_ids=[1])
