"""Pitch correction, host side (no GPU): the numpy statement (tests/pitch_tune_cases.py) on cases computed by hand,
`infer_offline.PitchTune`, jobs of four, five and six entries, `job_tunes` and `tune_tables`, `main.py`'s options, the symbol,
the binding's refusals and the bank's host state."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import pitch_tune_cases as PC
from conftest import ROOT
from test_bank_models_host import bank_model

A_MINOR = PC.A_MINOR


# ---- the statement, by hand -----------------------------------------------------------------------------------------------------
def test_an_exact_tie_takes_the_lower_note():
    """Mask {G, B}, a4 = 440: 220, 440 and 880 Hz are the As 57, 69 and 81 - log2 of a power of two is exact -, two semitones
    from the G below and from the B above: the G wins."""
    f0 = np.array([[220.0, 440.0, 880.0]], dtype=np.float32)
    for f, m in zip(f0[0], (57.0, 69.0, 81.0)):
        assert PC.offset(f, 440.0, PC.G_B) == (-2.0, m)
    out, corr, err = PC.tune_rows(f0, [PC.G_B], [[440.0, 1.0, 1.0]])
    assert not err and corr.tolist() == [[-2.0, -2.0, -2.0]]
    assert np.array_equal(out, (f0.astype(np.float64) * np.exp2(-2.0 / 12.0)).astype(np.float32))
    assert np.allclose(out[0], [195.9977, 391.9954, 783.9909], rtol=1e-6)                   # G3, G4, G5
    assert PC.offset(440.0, 440.0, 1 << 9) == (0.0, 69.0) and PC.offset(440.0, 440.0, 1 << 3)[0] == -6.0   # the tritone: down


def test_hard_tuning_lands_on_the_note():
    f0 = np.array([[150.0, 215.0, 335.0, 452.0, 61.0]], dtype=np.float32)
    out, corr, _ = PC.tune_rows(f0, [A_MINOR], [[440.0, 1.0, 1.0]])
    m = 69.0 + 12.0 * np.log2(out.astype(np.float64) / 440.0)
    assert np.abs(m - np.round(m)).max() < 1e-5 and np.round(m)[0].tolist() == [50.0, 57.0, 64.0, 69.0, 35.0]   # D3 A3 E4 A4 B1
    assert all((A_MINOR >> (int(n) % 12)) & 1 for n in np.round(m)[0]) and np.abs(corr).max() <= 0.5
    half, corr_half, _ = PC.tune_rows(f0, [A_MINOR], [[440.0, 0.5, 1.0]])                   # half the strength: half the way
    assert np.array_equal(corr_half, corr)
    assert np.allclose(12 * np.log2(half.astype(np.float64) / f0), corr / 2, atol=1e-5)


def test_off_returns_the_inputs_bits():
    f0 = np.array([[150.0, -0.0, np.nan, 215.0, np.inf, 1e-45]], dtype=np.float32)
    for mask, param in ((0, [440.0, 1.0, 1.0]), (A_MINOR, [440.0, 0.0, 0.3]), (0x1000, [440.0, 1.0, 1.0]), (0, [np.nan, 7.0, 0.0])):
        out, corr, err = PC.tune_rows(f0, [mask], [param])
        assert not err and PC.same_bits(out, f0) and not corr.any()
    out, corr, err = PC.tune_rows(f0, [A_MINOR], [[440.0, 1.0, 1.0]], owner=[1])           # an owner outside [0, J)
    assert not err and PC.same_bits(out, f0)
    for bad in ([0.0, 1.0, 1.0], [np.inf, 1.0, 1.0], [440.0, 1.5, 1.0], [440.0, 1.0, 0.0], [440.0, 1.0, np.nan]):
        out, corr, err = PC.tune_rows(f0, [A_MINOR], [bad])
        assert err and PC.same_bits(out, f0) and not corr.any()
    out, _, _ = PC.tune_rows(f0, [A_MINOR], [[440.0, 1.0, 1.0]], n_frames=[3])             # behind the count
    assert PC.same_bits(out[0, 1:], f0[0, 1:]) and out[0, 0] != f0[0, 0]


def test_a_reset_follows_an_unvoiced_frame():
    """d = +0.4, -0.3, [gap], +0.2, +0.2 at alpha = 0.5: c = 0.4, 0.05, -, 0.2 (not 0.125), 0.2."""
    m = np.array([56.6, 57.3, 0.0, 59.8, 59.8])
    f0 = (440.0 * 2 ** ((m - 69.0) / 12.0)).astype(np.float32)
    f0[2] = 0.0
    out, corr, _ = PC.tune_rows(f0[None], [1 << 9 | 1 << 0], [[440.0, 1.0, 0.5]])          # {A, C}: 57 and 60
    assert np.allclose(corr[0], [0.4, 0.05, 0.0, 0.2, 0.2], atol=1e-6) and corr[0, 2] == 0 and out[0, 2] == 0
    lead = np.concatenate([np.array([np.nan, -1.0], dtype=np.float32), f0])                 # the row's first voiced frame resets too
    assert np.allclose(PC.tune_rows(lead[None], [1 << 9 | 1 << 0], [[440.0, 1.0, 0.5]])[1][0, 2:], corr[0], atol=0)
    _, slow, _ = PC.tune_rows(np.full((1, 200), f0[0]), [1 << 9], [[440.0, 1.0, 0.05]])     # a constant d: c stays d
    assert np.allclose(slow, slow[0, 0], atol=1e-12)


def test_the_generator_holds_its_conditions():
    f0, gaps = PC.rows(130)
    assert gaps[0, 0] and gaps[1, 62] and gaps[1, 63] and gaps[2, 64] and gaps[3, 63:66].all() and gaps[4, 129] and not gaps[1, 0]
    voiced = f0[~gaps]
    assert voiced.min() >= 60 and voiced.max() <= 1000 and {0.0, -130.0, np.inf} <= set(f0[gaps].tolist()) and np.isnan(f0[gaps]).any()
    assert PC.counts(130).tolist() == [130, 129, 1, 86, 130] and PC.counts(1).tolist() == [1] * 5
    assert all(PC.m_is_robust(f, 440.0) for f in voiced) and PC.m_is_robust(880.0, 440.0)


# ---- PitchTune ------------------------------------------------------------------------------------------------------------------
def test_pitch_tune_scales_and_refusals():
    from infer_offline import PitchTune
    bits = lambda *pcs: sum(1 << p for p in pcs)  # noqa: E731
    assert PitchTune.scale("C", "major").mask == bits(0, 2, 4, 5, 7, 9, 11) == PitchTune.scale("A", "minor").mask == A_MINOR
    assert PitchTune.scale("A", "minor").notes == (0, 2, 4, 5, 7, 9, 11)
    assert PitchTune.scale(9, "major").mask == bits(9, 11, 1, 2, 4, 6, 8)
    assert PitchTune.scale("F#", "chromatic").mask == 0xfff
    assert PitchTune.scale("C", "major_pentatonic").mask == bits(0, 2, 4, 7, 9) == PitchTune.scale("A", "minor_pentatonic").mask
    assert PitchTune.scale("Bb", "minor_pentatonic").mask == bits(10, 1, 3, 5, 8)
    assert PitchTune.scale("D").mask == PitchTune.named("D major").mask == PitchTune.named("D").mask
    assert PitchTune(["A", 0, "c#", "Db", "B#"]).notes == (0, 1, 9) and PitchTune(range(12)).mask == 0xfff
    t = PitchTune.named("A minor", strength=0.5, retune=0.1, a4=442)
    assert (t.strength, t.retune, t.a4) == (0.5, 0.1, 442.0)
    mask, (a4, s, alpha) = t.setting(512 / 44100)
    assert mask == A_MINOR and (a4, s) == (442.0, 0.5) and alpha == pytest.approx(1 - math.exp(-512 / 44100 / 0.1), rel=1e-12)
    assert PitchTune([0], retune=0).setting(0.01)[1][2] == 1.0 and PitchTune([0], retune=1e-9).setting(0.01)[1][2] == 1.0
    assert 0 < PitchTune([0], retune=1e9).setting(0.01)[1][2] < 1e-10
    for notes in ([], (), "A", 5, None, [12], [-1], ["H"], ["A+"], [True], [1.5]):
        with pytest.raises(ValueError, match="PitchTune"):
            PitchTune(notes)
    for kw in (dict(strength=-0.1), dict(strength=1.1), dict(strength=float("nan")), dict(strength="1"), dict(retune=-1),
               dict(retune=float("inf")), dict(retune=float("nan")), dict(a4=0), dict(a4=-440), dict(a4=float("inf")), dict(a4=None),
               dict(strength=True)):
        with pytest.raises(ValueError, match="PitchTune"):
            PitchTune([0], **kw)
    for tonic, kind in (("A", "dorian"), ("H", "major"), (12, "minor")):
        with pytest.raises(ValueError, match="PitchTune.scale"):
            PitchTune.scale(tonic, kind)
    for text in ("", "A minor blues", None):
        with pytest.raises(ValueError, match="PitchTune.named"):
            PitchTune.named(text)
    for hop in (0, -1, float("nan")):
        with pytest.raises(ValueError, match="hop_seconds"):
            t.setting(hop)


# ---- jobs -----------------------------------------------------------------------------------------------------------------------
def test_jobs_of_four_five_and_six_entries():
    import infer_offline
    from infer_offline import FormantTimeline, PitchTune
    model = bank_model("CombSub", 2, 43)
    pieces = infer_offline.piece_table([[(0, 5120), (8192, 12288)]], 512.0)
    tune = PitchTune.scale("A", "minor")
    jobs = [(0, 0, 1, 0), (0, 0, 2, 3.0, 2), (0, 0, 1, -1, None, tune), (0, 0, 1, 0, FormantTimeline([(0, 1)]), None), (0, 0, 2, 1, 3, tune)]
    table = infer_offline.job_table(pieces, 1, jobs, [model])
    assert table == infer_offline.job_table(pieces, 1, [job[:4] for job in jobs], [model])   # the dict keeps its keys and values
    assert set(table) == {"rows", "piece_of_row", "model_of_job", "speakers", "key_factor", "starts_per_job", "keys"}
    assert infer_offline.job_tunes(jobs) == [None, None, tune, None, tune]
    formants = infer_offline.job_formants(jobs)
    assert formants[:3] == [None, 2.0, None] and isinstance(formants[3], FormantTimeline) and formants[4] == 3.0
    masks, params = infer_offline.tune_tables(infer_offline.job_tunes(jobs), 44100, 512)
    assert masks.dtype == torch.int32 and masks.tolist() == [0, 0, A_MINOR, 0, A_MINOR]
    alpha = 1 - math.exp(-512 / 44100 / 0.05)
    assert params.dtype == torch.float64 and tuple(params.shape) == (5, 3) and params[0].tolist() == [440.0, 0.0, 1.0]
    assert params[2].tolist() == pytest.approx([440.0, 1.0, alpha], rel=1e-12)
    empty = infer_offline.tune_tables([], 44100, 512)
    assert tuple(empty[0].shape) == (0,) and tuple(empty[1].shape) == (0, 3)
    for bad in ((0, 0, 1), (0, 0, 1, 0, None, tune, 1), 5):
        with pytest.raises(ValueError, match="must be"):
            infer_offline.job_table(pieces, 1, [bad], [model])
    for bad in ("A minor", 3, A_MINOR, [0, 2]):
        with pytest.raises(ValueError, match="job 1 must be .* with tune a PitchTune or None"):
            infer_offline.job_table(pieces, 1, [jobs[0], (0, 0, 1, 0, None, bad)], [model])
    with pytest.raises(ValueError, match="job 0: formant"):
        infer_offline.job_table(pieces, 1, [(0, 0, 1, 0, 30, tune)], [model])


def test_main_takes_a_tune():
    import main
    from infer_offline import PitchTune
    base = ["-m", "m.pt", "-i", "in.wav", "-o", "out.wav"]
    plain = main.parse_args(base)
    assert not any(hasattr(plain, name) for name in ("tune_scale", "tune_strength", "tune_retune_ms", "tune_a4"))
    assert main._cmd_tune(plain) is None
    cmd = main.parse_args(base + ["--tune_scale", "A minor", "--tune_strength", "0.8", "--tune_retune_ms", "20", "--tune_a4", "442"])
    t = main._cmd_tune(cmd)
    assert isinstance(t, PitchTune) and (t.mask, t.strength, t.a4) == (A_MINOR, 0.8, 442.0) and t.retune == pytest.approx(0.02)
    d = main._cmd_tune(main.parse_args(base + ["--tune_scale", "C"]))
    assert (d.mask, d.strength, d.retune, d.a4) == (A_MINOR, 1.0, 0.05, 440.0)
    assert main._job_entry(0, {"id": 2, "key": 3, "tune": {"scale": "A minor"}, "suffix": "a"}) == (2, 3.0)
    assert main._job_tune(0, {"suffix": "a"}) is None and main._job_tune(0, {"suffix": "a"}, t) is t
    e = main._job_tune(1, {"tune": {"notes": ["C", 4, "G"], "strength": 0.5, "retune_ms": 0, "a4": 415}, "suffix": "b"}, t)
    assert (e.notes, e.strength, e.retune, e.a4) == ((0, 4, 7), 0.5, 0.0, 415.0)
    for bad in ("A minor", {"scale": "A minor", "notes": [0]}, {}, {"strength": 1}, {"scale": "A minor", "speed": 1}):
        with pytest.raises(ValueError, match="entry 2"):
            main._job_tune(2, {"tune": bad, "suffix": "c"})
    with pytest.raises(ValueError, match="PitchTune"):
        main._job_tune(3, {"tune": {"scale": "A minor", "strength": 2}, "suffix": "d"})


# ---- the symbol and the binding -------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_bound_and_exported(lib_path):
    import hipddsp
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddsp_amd.h")).read(), flags=re.S)
    assert re.findall(r"\b(ddsp_\w+)\s*\(", text).count("ddsp_f0_tune") == 1 and hasattr(ctypes.CDLL(lib_path), "ddsp_f0_tune")
    proto = re.search(r"int ddsp_f0_tune\((.*?)\);", text, flags=re.S).group(1)
    assert len(proto.split(",")) == len(hipddsp.SIGNATURES["ddsp_f0_tune"][1]) == 11
    assert hipddsp.ABI_VERSION == 8 and ctypes.CDLL(lib_path).ddsp_abi_version() == 8       # a new symbol beside unchanged ones
    common = open(os.path.join(ROOT, "ddsp-svc-official_amd", "csrc", "common.h")).read()
    assert re.search(r"#define DDSP_DEV_ERR_TUNE 7\b", common)


def test_the_binding_refuses_before_any_launch():
    import hipddsp
    ctx = object.__new__(hipddsp.Context)                      # no device: every refusal below comes before the library call
    good = dict(f0=torch.zeros(2, 5), mask=torch.zeros(3, dtype=torch.int32), param=torch.zeros(3, 3, dtype=torch.float64))
    cases = [dict(f0=torch.zeros(2, 5, dtype=torch.float64)), dict(f0=torch.zeros(10)), dict(f0=torch.zeros(5, 2).t()),
             dict(f0=torch.zeros(2, 5, 2)), dict(f0=torch.zeros(0, 5)), dict(f0=np.zeros((2, 5), dtype=np.float32))]
    for case in cases:
        with pytest.raises(ValueError, match="f0_tune_: f0 must be"):
            ctx.f0_tune_(**{**good, **case})
    with pytest.raises(ValueError, match="f0_tune_: f0 must be"):                          # a CPU tensor is no device tensor
        ctx.f0_tune_(**good)


# ---- the bank's host state ------------------------------------------------------------------------------------------------------
def _bank(model, n=3, **kw):
    import realtime
    return realtime.StreamBank(model, n, 44100, 0.1, 0.04, "cpu", buffer_num=4, use_graph=False, max_mix=3, **kw)


def test_bank_tune_rows_and_refusals(lib_path):
    from infer_offline import PitchTune
    model = bank_model("CombSub", 4, 43)
    tune = PitchTune.scale("A", "minor", strength=0.5, retune=0.02)
    plain = _bank(model)
    assert plain.tune_mask is None and plain.tune_param is None and plain._full.tune_term is None
    with pytest.raises(ValueError, match="without tune=True"):
        plain.set_tune(0, tune)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="tune must be True or False"):
            _bank(model, tune=bad)
    bank = _bank(model, tune=True, active_widths=(1, 2), pitch_breakpoints=2, formant=True)
    assert bank.tune_mask.tolist() == [0, 0, 0] and bank.tune_mask.dtype == torch.int32
    assert bank.tune_param.dtype == torch.float64 and bank.tune_param.tolist() == [[440.0, 0.0, 1.0]] * 3
    assert bank._full.tune_term == (bank.tune_mask, bank.tune_param, None)
    for W, rows in sorted(bank._compact.items()):
        assert rows.tune_term[0] is bank.tune_mask and rows.tune_term[1] is bank.tune_param and rows.tune_term[2] is rows.rows
    bank.set_tune(1, tune)
    alpha = 1 - math.exp(-bank.hop_size / 44100 / 0.02)
    assert bank.tune_mask.tolist() == [0, A_MINOR, 0] and bank.tune_param[1].tolist() == pytest.approx([440.0, 0.5, alpha], rel=1e-12)
    assert bank.graph_builds == 0
    for slot, t in ((3, tune), (-1, tune), (True, tune), (0, "A minor"), (0, A_MINOR), (0, 0)):
        with pytest.raises(ValueError):
            bank.set_tune(slot, t)
    assert bank.tune_mask.tolist() == [0, A_MINOR, 0]                                       # a refused call wrote nothing
    bank.set_tune(2, tune)
    bank.set_tune(1, None)
    assert bank.tune_mask.tolist() == [0, 0, A_MINOR] and bank.tune_param[1].tolist() == [440.0, 0.0, 1.0]
    bank.reset(2)
    assert bank.tune_mask.tolist() == [0, 0, 0]
    two = _bank(None, models=[model, model], tune=True)                                      # works with `models=`
    two.set_tune(0, tune)
    assert two.tune_mask.tolist() == [A_MINOR, 0, 0]
