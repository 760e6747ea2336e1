"""Host side of the enhancer stage of the stream bank: the key threshold table against the reference's numpy expression, the
lengths of `enhancer.KeyedPlan` against `Enhancer.batch_lengths`, the new symbols in the header and the binding, and the
refusals of `StreamBank` / `Enhancer.enhance_keyed`, which are raised before anything needs a device."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import glue_cases as GC
import synthetic
from conftest import ROOT

NEW = ["ddsp_enhancer_keys", "ddsp_resample_keyed_plan", "ddsp_resample_keyed_plan_destroy", "ddsp_resample_keyed_length",
       "ddsp_resample_keyed", "ddsp_retime_f0_keyed"]


def _reference_key(f, max_key=12):
    """`enhancer.py:34-38` ('auto') for the f0 maximum `f`, capped at max_key: the quotient in fp32, the rest as numpy does it."""
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.ceil(12 * np.log2(float(np.float32(f) / np.float32(760))))
    return int(min(max_key, max(0, k))) if f > 0 else 0


def test_threshold_table_reproduces_the_reference_expression(lib_path):
    import hipddsp
    thr = hipddsp.key_thresholds(12)
    assert thr.dtype == np.float32 and thr.shape == (13,) and thr[0] == 1.0 and thr[12] == 2.0
    for k in range(13):                      # the largest fp32 value <= 2^(k/12)
        assert float(thr[k]) <= 2.0 ** (k / 12.0) < float(np.nextafter(thr[k], np.float32(4)))
    cases = [0.0, -3.0, 760.0, 1520.0]
    for k in range(13):
        edge = np.float32(760.0 * 2.0 ** (k / 12.0))
        lo = hi = edge
        cases.append(float(edge))
        for _ in range(4):
            lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(1e9))
            cases += [float(lo), float(hi)]
    rng = np.random.Generator(np.random.PCG64(760))
    cases += [float(np.float32(v)) for v in rng.uniform(50.0, 4000.0, 3000)]
    for max_key in (12, 5, 0):
        t = hipddsp.key_thresholds(max_key)
        assert np.array_equal(t, thr[:max_key + 1])
        bad = [(f, hipddsp.key_from_thresholds(f, t), _reference_key(f, max_key)) for f in cases
               if hipddsp.key_from_thresholds(f, t) != _reference_key(f, max_key)]
        assert not bad, bad[:5]
    import realtime
    for f in cases:                          # the helper the solo renderer uses agrees where the cap does not bind
        if 0 < f <= 1520.0:
            assert hipddsp.key_from_thresholds(f, thr) == realtime.auto_key(f)


def _enhancer(tmp_path):
    from enhancer import Enhancer
    with open(tmp_path / "config.json", "w") as fh:
        json.dump(dict(GC.NSF_CONFIG), fh)
    torch.save({"generator": GC.nsf_state_dict()}, tmp_path / "model")
    return Enhancer("nsf-hifigan", str(tmp_path / "model"), device="cuda")


@pytest.mark.parametrize("device_sr", [44100, 48000])
def test_keyed_plan_lengths(lib_path, tmp_path, device_sr):
    """Model rate 44 100 with a 44 100 and a 48 000 Hz device (the bank's window, so its frames, differ): per key the plan's row
    is `batch_lengths` at that key's working rate."""
    import realtime
    enh = _enhancer(tmp_path)
    assert enh.enhancer_sample_rate == 44100
    z = realtime.bank_sizes(device_sr, 0.2, 0.04, 4, 512, 44100)
    T, Fr = z["frames"] * 512, z["frames"]
    for silence in (0, z["silence_front"]):
        plan = enh.keyed_plan(T, Fr, 44100, 512, silence, 12)
        cut_frames = int(silence * 44100 / 512)
        assert (plan.cut_frames, plan.cut_samples) == (cut_frames, cut_frames * 512) and plan.T_cut == T - cut_frames * 512
        assert (cut_frames > 0) == (silence > 0)
        assert len(plan.lengths) == len(plan.rates) == 13 and plan.rates[0] == 44100 and plan.rates[12] == 88200
        for k in range(13):
            rate = 100 * int(np.round(44100 * 2 ** (k / 12) / 100))
            assert plan.rates[k] == rate == enh._working_rate(k, None)[0]
            assert plan.lengths[k] == tuple(enh.batch_lengths(plan.T_cut, 44100, rate))
            assert plan.n_out[k] == plan.lengths[k][4] + plan.front_pad
        assert plan.widths == tuple(max(r[i] for r in plan.lengths) for i in range(5))
        assert len({r[4] for r in plan.lengths}) > 1, "n_out must differ between keys"
        assert plan.front_pad == (int(np.round(44100 * (cut_frames * 512 / 44100))) if cut_frames else 0)
    assert enh.keyed_plan(T, Fr, 44100, 512, 0, 3).lengths == enh.keyed_plan(T, Fr, 44100, 512, 0, 12).lengths[:4]


def test_new_symbols_declared_exported_and_bound(lib_path):
    """(The ABI number stays at 7: the new entry points stand beside unchanged ones, and tests/test_hubert_ragged_host.py and
    tests/test_crepe_host.py pin 7.  Header, library and binding must agree.)"""
    import hipddsp
    lib = hipddsp.load_library()
    text = open(os.path.join(ROOT, "include", "ddsp_amd.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in hipddsp.SIGNATURES, name
        assert getattr(lib, name).argtypes == hipddsp.SIGNATURES[name][1]
    with open(os.path.join(ROOT, "ddsp-svc-official_amd", "csrc", "ctx.hip")) as fh:
        src = int(re.search(r"#define DDSP_ABI_VERSION (\d+)", fh.read()).group(1))
    assert hipddsp.ABI_VERSION == src == lib.ddsp_abi_version()
    for m in ("enhancer_keys", "resample_keyed", "resample_plan"):
        assert hasattr(hipddsp.Context, m), m
    assert "keyed" in inspect.signature(hipddsp.Context.retime_f0).parameters
    from enhancer import Enhancer
    sig = inspect.signature(Enhancer.enhance_keyed).parameters
    assert [p for p in sig][1:] == ["audio", "sample_rate", "f0", "hop_size", "adaptive_key", "silence_front", "max_key", "rand_ini", "plan"]
    import realtime
    for p in ("enhancer", "enhancer_adaptive_key", "enhancer_max_key"):
        assert p in inspect.signature(realtime.StreamBank.__init__).parameters
    assert hasattr(realtime.StreamBank, "set_enhancer_key")


def test_refusals_come_before_any_device_call(lib_path, tmp_path, monkeypatch):
    """A `hipddsp.Context` cannot be made here (no device): every refusal below must be raised before one is asked for."""
    import hipddsp
    import realtime
    monkeypatch.setattr(hipddsp, "context_for", lambda device: pytest.fail("a refusal reached the device"))
    enh = _enhancer(tmp_path)
    model, _ = synthetic.build_model("CombSub", seed=43)
    bank = lambda **kw: realtime.StreamBank(model, 3, 44100, 0.2, 0.04, "cuda", buffer_num=4, use_graph=False, enhancer=enh, **kw)
    for kw in (dict(enhancer_adaptive_key="automatic"), dict(enhancer_adaptive_key=13), dict(enhancer_adaptive_key=-1),
               dict(enhancer_adaptive_key=6, enhancer_max_key=5), dict(enhancer_adaptive_key=2.5), dict(enhancer_max_key=13),
               dict(enhancer_max_key=-1), dict(enhancer_max_key=2.0), dict(enhancer_max_key=True)):
        with pytest.raises(ValueError):
            bank(**kw)
            pytest.fail(f"{kw} was accepted")

    class Odd:
        """An enhancer whose rate the resampler cannot pair with the model's 44 100 Hz (reduced rates >= 65536)."""
        enhancer_sample_rate, enhancer_hop_size = 99991, 512
        _front_cut = staticmethod(enh._front_cut)
        check_key_request = staticmethod(enh.check_key_request)
        keyed_plan = lambda self, *a: __import__("enhancer").KeyedPlan(self, *a)

        def _working_rate(self, key, f0):
            return type(enh)._working_rate(self, key, f0)

    with pytest.raises(ValueError):
        realtime.StreamBank(model, 3, 44100, 0.2, 0.04, "cuda", buffer_num=4, use_graph=False, enhancer=Odd())
    audio, f0 = torch.zeros(2, 4096), torch.full((2, 8, 1), 220.0)
    for kw in (dict(adaptive_key="automatic"), dict(adaptive_key=13), dict(adaptive_key=4, max_key=3), dict(max_key=13),
               dict(adaptive_key=-2), dict(adaptive_key=torch.zeros(2, dtype=torch.int64)), dict(adaptive_key=torch.zeros(3, dtype=torch.int32)),
               dict(silence_front=1.0)):
        with pytest.raises(ValueError):
            enh.enhance_keyed(audio, 44100, f0, 512, **kw)
            pytest.fail(f"{kw} was accepted")
    with pytest.raises(ValueError):
        enh.enhance_keyed(audio, 44100, f0, 512, plan=enh.keyed_plan(4096, 9, 44100, 512))      # another geometry
    with pytest.raises(ValueError):
        enh.enhance_keyed(audio[0], 44100, f0, 512)
    with pytest.raises(RuntimeError):                                                            # well-formed: no CPU fallback
        enh.enhance_keyed(audio, 44100, f0, 512)
