"""Host side of `realtime.StreamBank(models=...)`, a bank whose slots each name one of M models: the ladder of `model_widths`,
the refusals of the constructor (models that disagree in sampling rate, block size, unit width or device), `set_model` and the
per-model speaker check, all raised before anything needs a device, and the two new row movers in the header, the library and
the binding."""
import inspect
import os
import re

import pytest
import torch

import synthetic
from conftest import ROOT

NEW = ["ddsp_bank_features_gather", "ddsp_bank_signal_scatter"]
S = 4


def bank_model(kind, n_spk, seed, device="cpu", **over):
    """A seeded random-weight synthesiser of `synthetic.MODEL_CFG[kind]` with `n_spk` speakers (and any field of `over`)."""
    from ddsp.vocoder import CombSub, CombSubFast, Sins
    cfg = dict(synthetic.MODEL_CFG[kind], n_spk=n_spk, **over)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        if kind == "CombSub":
            m = CombSub(cfg["sampling_rate"], cfg["block_size"], cfg["n_mag_allpass"], cfg["n_mag_harmonic"], cfg["n_mag_noise"],
                        cfg["n_unit"], cfg["n_spk"])
        elif kind == "Sins":
            m = Sins(cfg["sampling_rate"], cfg["block_size"], cfg["n_harmonics"], cfg["n_mag_allpass"], cfg["n_mag_noise"],
                     cfg["n_unit"], cfg["n_spk"])
        else:
            m = CombSubFast(cfg["sampling_rate"], cfg["block_size"], cfg["n_unit"], cfg["n_spk"])
    finally:
        torch.random.set_rng_state(state)
    return m.to(device).eval()


@pytest.fixture(scope="module")
def pair(lib_path):
    return bank_model("CombSub", 1, 43), bank_model("Sins", 3, 44)


def _bank(model, n=S, **kw):
    """A bank on the CPU: its state is plain tensors, and no call that passes the refusals could run."""
    import realtime
    return realtime.StreamBank(model, n, 44100, 0.2, 0.04, "cpu", buffer_num=4, use_graph=False, **kw)


def test_model_widths_default_and_refusals(pair):
    import realtime
    assert [realtime.default_model_widths(n) for n in (1, 2, 3, 4, 5, 16)] == \
        [(1,), (1, 2), (1, 2, 3), (1, 2, 4), (1, 2, 4, 5), (1, 2, 4, 8, 16)]
    a, b = pair
    plain = _bank(a)
    assert plain.model_widths is None and plain.models == [a] and plain._model_rows is None and plain._batch is None
    bank = _bank(None, models=[a, b])
    assert bank.model_widths == (1, 2, 4) and bank.models == [a, b] and bank.model is a and bank.model_of_slot == [0] * S
    assert _bank(a, models=[a, b]).model is a                           # (the positional model may name model 0)
    assert _bank(None, models=[a, b], model_widths=(2,)).model_widths == (2, 4)
    assert _bank(None, models=[a, b], model_widths=()).model_widths == (4,)
    assert _bank(None, models=(a,), model_widths=(1, 4)).model_widths == (1, 4)
    assert sorted(bank._model_rows[1]) == [1, 2, 4] and len(bank._model_rows) == 2 and bank.graph_builds == 0
    for bad in ((2, 1), (1, 1), (0, 2), (1, 5), (True, 2), (1.0, 2), 2, "12"):
        with pytest.raises(ValueError, match="model_widths"):
            _bank(None, models=[a, b], model_widths=bad)
            pytest.fail(f"{bad!r} was accepted")
    with pytest.raises(ValueError, match="model_widths"):
        _bank(a, model_widths=(1, 2))                                   # (a ladder without models)
    for bad in ([], (), a, "ab"):
        with pytest.raises(ValueError, match="models"):
            _bank(None, models=bad)
    with pytest.raises(ValueError, match="models\\[0\\]"):
        _bank(b, models=[a, b])                                         # (a second meaning of the positional model)


def test_mismatched_models_are_refused_before_any_device_call(pair, monkeypatch):
    import hipddsp
    monkeypatch.setattr(hipddsp, "context_for", lambda device: pytest.fail("a refusal reached the device"))
    a, _ = pair
    cases = {"sampling_rate": bank_model("Sins", 3, 44, sampling_rate=48000), "block_size": bank_model("Sins", 3, 44, block_size=256),
             "n_unit": bank_model("Sins", 3, 44, n_unit=4), "device": bank_model("Sins", 3, 44, device="meta")}
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: pytest.fail("a refusal allocated state"))
    for field, odd in cases.items():
        with pytest.raises(ValueError, match=r"models\[2\]\.%s " % field):
            _bank(None, models=[a, a, odd])
            pytest.fail(f"a model of another {field} was accepted")


def test_set_model_and_the_speaker_of_the_slots_own_model(pair):
    a, b = pair                                                         # n_spk 1 and 3
    bank = _bank(None, models=[a, b])
    state = lambda: (list(bank.model_of_slot), bank.spk_ids.clone(), bank.spk_w.clone())
    before = state()
    bad = [lambda: bank.set_model(S, 1), lambda: bank.set_model(-1, 1), lambda: bank.set_model(True, 1), lambda: bank.set_model(0, 2),
           lambda: bank.set_model(0, -1), lambda: bank.set_model(0, True), lambda: bank.set_model(0, 1.0),
           lambda: bank.set_model(0, 1, spk_id=4), lambda: bank.set_model(0, 1, spk_id=0), lambda: bank.set_model(0, 0, spk_id=2),
           lambda: bank.set_model(0, 1, spk_mix_dict={1: 0.5, 4: 0.5}), lambda: bank.set_model(0, 1, spk_mix_dict={}),
           lambda: bank.set_speaker(1, spk_id=2)]                       # (slot 1 is on model 0, which has one speaker)
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {i} did not raise")
    after = state()
    assert after[0] == before[0] and torch.equal(after[1], before[1]) and torch.equal(after[2], before[2])
    bank.set_model(1, 1, spk_id=3)
    bank.set_model(3, 1, spk_mix_dict={2: 0.25, 3: 0.75})
    assert bank.model_of_slot == [0, 1, 0, 1] and bank.spk_ids[1].tolist() == [3, 1, 1, 1] and bank.spk_w[1].tolist() == [1, 0, 0, 0]
    assert bank.spk_ids[3].tolist() == [2, 3, 1, 1] and bank.spk_w[3].tolist() == [0.25, 0.75, 0, 0]
    bank.set_speaker(1, spk_id=2)                                       # valid for model 1 ...
    with pytest.raises(ValueError):
        bank.set_speaker(0, spk_id=2)                                   # ... and still outside model 0's one speaker
    bank.reset(1)
    assert bank.model_of_slot == [0, 1, 0, 1]                           # (a reset keeps the model)
    bank.set_model(1, 0)
    assert bank.model_of_slot == [0, 0, 0, 1] and bank.spk_ids[1].tolist() == [1, 1, 1, 1] and bank.graph_builds == 0
    plain = _bank(a)
    plain.set_model(2, 0)                                               # (a bank of one model has model 0 alone)
    with pytest.raises(ValueError):
        plain.set_model(2, 1)


def test_new_symbols_declared_exported_and_bound(lib_path):
    """(The ABI number stays at 8: the two entry points stand beside unchanged ones.)"""
    import graphed
    import hipddsp
    import realtime
    lib = hipddsp.load_library()
    with open(os.path.join(ROOT, "include", "ddsp_amd.h")) as fh:
        text = fh.read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in hipddsp.SIGNATURES, name
        assert getattr(lib, name).argtypes == hipddsp.SIGNATURES[name][1]
        proto = re.search(r"\bint %s\s*\(([^;]*)\);" % name, text).group(1)
        assert len(proto.split(",")) == len(hipddsp.SIGNATURES[name][1]), name
    assert hipddsp.ABI_VERSION == 8 == lib.ddsp_abi_version()
    for method, name in (("bank_features_gather_", NEW[0]), ("bank_signal_scatter_", NEW[1])):
        called = re.findall(r"call\(\s*\"(ddsp_\w+)\"", inspect.getsource(getattr(hipddsp.Context, method)))
        assert called == [name], (method, called)
    params = inspect.signature(realtime.StreamBank.__init__).parameters
    assert "models" in params and "model_widths" in params and params["models"].default is None
    assert list(inspect.signature(realtime.StreamBank.set_model).parameters) == ["self", "slot", "k", "spk_id", "spk_mix_dict"]
    for call in (realtime.StreamBank.push_audio, realtime.StreamBank.push_block):
        assert list(inspect.signature(call).parameters)[-3:] == ["noise", "rand_ini", "active"]
    assert issubclass(graphed.GraphedModelRows, graphed.GraphedSynth) and issubclass(graphed.GraphedSynth, graphed._Captured)
