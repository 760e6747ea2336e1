"""The formant shift, host side (no GPU): the properties of the numpy statement (tests/formant_cases.py) that the GPU tests hold
`ddsp_ctrl_warp` to, `infer_offline.FormantTimeline`, jobs of four and five entries, the bounds, `main.py`'s options, the
binding's refusals and the bank's host state."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import formant_cases as FC
from conftest import ROOT
from test_bank_models_host import bank_model


# ---- the statement --------------------------------------------------------------------------------------------------------------
def _bump(n, at, origin=0, width=3.0):
    j = np.arange(n, dtype=np.float64) + origin
    return (-8.0 + 6.0 * np.exp(-0.5 * ((j - at) / width) ** 2)).astype(np.float32)        # a log-magnitude


def test_identity_returns_the_inputs_bits():
    x = np.random.Generator(np.random.PCG64(1)).standard_normal(513).astype(np.float32)
    x[[0, 7, 100, 512]] = [-0.0, np.inf, np.nan, -np.inf]
    for origin in (0, 1):
        assert FC.same_bits(FC.warp_segment(x, 1.0, origin), x)
    assert FC.same_bits(FC.warp_segment(x[:1], FC.factor(7), 0), x[:1])                   # n == 1: a copy


def test_direction_of_the_shift():
    x = _bump(256, 40)
    assert int(np.argmax(FC.warp_segment(x, FC.factor(12), 0))) == 80
    assert int(np.argmax(FC.warp_segment(x, FC.factor(-12), 0))) == 20
    h = _bump(64, 8, origin=1)                                                           # column j is harmonic j + 1
    assert int(np.argmax(h)) + 1 == 8 and int(np.argmax(FC.warp_segment(h, FC.factor(12), 1))) + 1 == 16


def test_clamps_hold_the_ends():
    x = np.arange(1, 33, dtype=np.float32)
    down = FC.warp_segment(x, FC.factor(-12), 0)                                         # reads at 2 j: the top half clamps
    assert FC.same_bits(down[16:], np.full(16, x[-1])) and down[0] == x[0] and down[5] == x[10]
    up = FC.warp_segment(x, FC.factor(12), 1)                                            # harmonics: (j + 1) / 2 - 1 < 0 at j = 0
    assert up[0] == x[0] and up[1] == x[0] and up[3] == x[1] and up[2] == np.float32(1.5)


def test_rows_counts_tables_and_bad_factors():
    ctrl = np.random.Generator(np.random.PCG64(2)).standard_normal((6, 14)).astype(np.float32)
    segs = [(0, 5, 1), (7, 2, 0)]
    out, err = FC.warp_rows(ctrl, segs, [1.5, 0.0], 3, n_frames=[2, 3])
    assert err and FC.same_bits(out[2:], ctrl[2:]) and not FC.same_bits(out[:2], ctrl[:2])   # frame 2 of row 0; the bad row 1
    assert FC.same_bits(out[:, 5:7], ctrl[:, 5:7]) and FC.same_bits(out[:, 9:], ctrl[:, 9:])
    out, err = FC.warp_rows(ctrl, segs, [1.5, 2.0, 0.5], 3, slot_of_row=[-1, 2])
    assert not err and FC.same_bits(out[:3], ctrl[:3])
    assert FC.same_bits(out[3:, :5], np.stack([FC.warp_segment(r[:5], 0.5, 1) for r in ctrl[3:]]))
    out, _ = FC.warp_rows(ctrl, segs, [1.0, 1.0, 2.0, 1.0, 1.0, 1.0], 3)                      # a factor per frame
    assert FC.same_bits(np.delete(out, 2, 0), np.delete(ctrl, 2, 0)) and not FC.same_bits(out[2], ctrl[2])


# ---- FormantTimeline, jobs, bounds ----------------------------------------------------------------------------------------------
def test_formant_timeline_validation_mirrors_key_timeline():
    from infer_offline import FormantTimeline, KeyTimeline
    tl = FormantTimeline([(0, 0), (0.5, 2.0), [1.25, -3]])
    assert tl.points == [(0.0, 0.0), (0.5, 2.0), (1.25, -3.0)]
    assert tl.frames(44100, 512) == KeyTimeline(tl.points).frames(44100, 512) == ([0, 43, 108], [0.0, 2.0, -3.0])
    bad = [None, [], (), "x", [(0, 1, 2)], [3.0], [(-0.1, 0)], [(float("nan"), 0)], [(float("inf"), 0)], [(True, 0)], [("0", 0)],
           [(0.5, 0), (0.4, 0)], [(0, float("nan"))], [(0, float("inf"))], [(0, "2")], [(0, None)], [(0, True)], [(0, {1: 1.0})],
           [(0, 24.5)], [(0, 1), (1, -25)]]
    for points in bad:
        with pytest.raises(ValueError, match="FormantTimeline"):
            FormantTimeline(points)
            pytest.fail(f"{points!r} was accepted")
    assert FormantTimeline([(0, 24), (1, -24)]).points[1] == (1.0, -24.0)
    with pytest.raises(ValueError, match="FormantTimeline: points 0 and 1 .* both land on frame 9"):
        FormantTimeline([(0.100, 0), (0.101, 2)]).frames(44100, 512)


PIECES = [(0, 0, 43, 0, 22016), (0, 77, 35, 39424, 17920), (1, 0, 60, 0, 30720)]


@pytest.fixture(scope="module")
def models(lib_path):
    return [bank_model("CombSub", 2, 43), bank_model("Sins", 2, 44)]


def test_jobs_of_four_and_five_entries(models):
    from infer_offline import FormantTimeline, KeyTimeline, formant_tables, job_formants, job_table, key_tables
    four = [(0, 0, 1, 0), (0, 1, {1: 0.25, 2: 0.75}, 3), (1, 0, 2, -2.5)]
    tl = FormantTimeline([(0.0, 0), (1.0, 2)])
    five = [four[0] + (2,), four[1], four[2] + (tl,)]
    want, got = job_table(PIECES, 2, four, models), job_table(PIECES, 2, five, models)
    assert set(got) == set(want) and all(got[name] == want[name] for name in want)        # the tables carry no formant
    assert job_formants(four) == [None, None, None] and job_formants([four[0] + (None,)]) == [None]
    shifts = job_formants(five)
    assert shifts[0] == 2.0 and isinstance(shifts[0], float) and shifts[1] is None and shifts[2] is tl
    for a, b in zip(formant_tables(shifts, 44100, 512), key_tables([2.0, 0.0, KeyTimeline(tl.points)], 44100, 512)):
        assert torch.equal(a, b)
    assert formant_tables(shifts, 44100, 512)[3].tolist() == [FC.factor(2), 1.0, 1.0, FC.factor(2)]
    for formant, what in ((24.5, "24"), (-25, "24"), (float("nan"), "finite"), (float("inf"), "finite"), ("2", "finite"),
                          (True, "finite"), (KeyTimeline([(0, 1)]), "FormantTimeline"),
                          (FormantTimeline([(0.100, 0), (0.101, 2)]), "both land on frame 9")):
        with pytest.raises(ValueError, match=f"job 1: .*{what}"):
            job_table(PIECES, 2, [four[0], (0, 0, 1, 0, formant)], models)
            pytest.fail(f"{formant!r} was accepted")
    with pytest.raises(ValueError, match="job 0: key must be"):
        job_table(PIECES, 2, [(0, 0, 1, tl)], models)                                     # a formant timeline is no key
    for job in ((0, 0, 1), (0, 0, 1, 0, 2, 3)):
        with pytest.raises(ValueError, match="job 0 must be"):
            job_table(PIECES, 2, [job], models)


def test_semitone_bounds():
    import hipddsp
    assert hipddsp.formant_factor(0) == 1.0 and hipddsp.formant_factor(12) == 2.0 and hipddsp.formant_factor(-24) == 0.25
    assert np.float32(hipddsp.formant_factor(3)) == FC.factor(3)
    for s in (24.001, -25, float("nan"), float("inf"), -float("inf"), "3", None, True):
        with pytest.raises(ValueError, match="formant"):
            hipddsp.formant_factor(s)
    m = bank_model("CombSub", 2, 43)
    z = torch.zeros(1, 4, 256), torch.full((1, 4, 1), 200.0), torch.zeros(1, 4), torch.ones(1, 1, dtype=torch.int64)
    with torch.no_grad():
        for s in (25, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="formant"):
                m.forward_formant(*z, s)
        with pytest.raises(ValueError, match="formant"):
            m.forward_formant(*z, torch.ones(1, 5))                                       # (B, Fr) = (1, 4)
        with pytest.raises(ValueError, match="formant"):
            m.forward_formant(*z, torch.ones(1, dtype=torch.float64))
    assert m._formant_segments() == [(256, 512, 0), (768, 256, 0)]
    assert bank_model("Sins", 2, 44)._formant_segments() == [(0, 128, 1), (384, 256, 0)]
    assert bank_model("CombSubFast", 2, 45)._formant_segments() == [(0, 513, 0), (1026, 513, 0)]


# ---- main.py --------------------------------------------------------------------------------------------------------------------
def test_main_parses_the_shift_and_the_jobs_entries():
    import main
    from infer_offline import FormantTimeline
    base = ["-m", "model.pt", "-i", "in.wav", "-o", "out.wav"]
    assert "formant_shift_key" not in vars(main.parse_args(base))                         # a plain call's namespace is the reference's
    assert main.parse_args(base + ["--formant_shift_key", "2.5"]).formant_shift_key == "2.5"
    assert main._job_entry(0, {"id": 2, "key": 3, "formant": 2, "suffix": "a"}) == (2, 3.0)
    assert main._job_formant(0, {"formant": 2, "suffix": "a"}) == 2.0 and main._job_formant(1, {"suffix": "b"}) is None
    assert main._job_formant(2, {"suffix": "c"}, 1.5) == 1.5 and main._job_formant(3, {"formant": 0, "suffix": "d"}, 1.5) is None
    tl = main._job_formant(4, {"formant_timeline": [{"at": 0, "formant": 0}, {"at": 1.5, "formant": -2}], "suffix": "e"})
    assert isinstance(tl, FormantTimeline) and tl.points == [(0.0, 0.0), (1.5, -2.0)]
    assert main._job_entry(4, {"formant_timeline": [{"at": 0, "formant": 0}], "suffix": "e"}) == (1, 0.0)
    with pytest.raises(ValueError, match="entry 5 takes formant or formant_timeline"):
        main._job_formant(5, {"formant": 1, "formant_timeline": [{"at": 0, "formant": 1}], "suffix": "f"})
    for points in ([], {"at": 0, "formant": 1}, [{"at": 0}], [{"at": 0, "key": 1}], [(0, 1)], None):
        with pytest.raises(ValueError, match="entry 6: formant_timeline is a non-empty list"):
            main._job_formant(6, {"formant_timeline": points, "suffix": "g"})
    with pytest.raises(ValueError, match="FormantTimeline"):
        main._job_formant(7, {"formant_timeline": [{"at": 0, "formant": 30}], "suffix": "h"})


# ---- the symbol and the binding -------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_bound_and_exported(lib_path):
    import hipddsp
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddsp_amd.h")).read(), flags=re.S)
    assert re.findall(r"\b(ddsp_\w+)\s*\(", text).count("ddsp_ctrl_warp") == 1 and hasattr(ctypes.CDLL(lib_path), "ddsp_ctrl_warp")
    proto = re.search(r"int ddsp_ctrl_warp\((.*?)\);", text, flags=re.S).group(1)
    assert len(proto.split(",")) == len(hipddsp.SIGNATURES["ddsp_ctrl_warp"][1]) == 13
    assert hipddsp.ABI_VERSION == 8 and ctypes.CDLL(lib_path).ddsp_abi_version() == 8       # a new symbol beside unchanged ones


def test_the_binding_refuses_before_any_launch():
    import hipddsp
    ctx = object.__new__(hipddsp.Context)                      # no device: every refusal below comes before the library call
    ctrl, one = torch.zeros(6, 14), torch.ones(2)
    seg = [(0, 5, 1)]
    cases = [
        (dict(ctrl2d=ctrl.double()), "ctrl2d"), (dict(ctrl2d=torch.zeros(6)), "ctrl2d"), (dict(ctrl2d=ctrl.t()), "ctrl2d"),
        (dict(Fr=4), "multiple of Fr"), (dict(Fr=0), "multiple of Fr"),
        (dict(segments=[]), "1 to 3 triples"), (dict(segments=seg * 4), "1 to 3 triples"), (dict(segments=[(0, 5)]), "1 to 3 triples"),
        (dict(segments=[(0, 5.0, 1)]), "1 to 3 triples"), (dict(segments=[(10, 5, 0)]), "inside the row"),
        (dict(segments=[(-1, 5, 0)]), "inside the row"), (dict(segments=[(0, 0, 0)]), "inside the row"),
        (dict(segments=[(0, 5, 2)]), "inside the row"),
        (dict(factor=one.double()), "factor"), (dict(factor=torch.ones(3)), "factor"), (dict(factor=torch.ones(3, 2)), "factor"),
        (dict(factor=[1.0, 1.0]), "factor"),
        (dict(slot_of_row=torch.zeros(2, dtype=torch.int64)), "slot_of_row"), (dict(slot_of_row=torch.zeros(3, dtype=torch.int32)), "slot_of_row"),
        (dict(slot_of_row=torch.zeros(2, dtype=torch.int32), factor=torch.ones(2, 3)), "one per slot"),
        (dict(n_dev=torch.ones(2, dtype=torch.int64)), "n_dev"), (dict(n_dev=torch.ones(3, dtype=torch.int32)), "n_dev"),
    ]
    for over, what in cases:
        kw = dict(ctrl2d=ctrl, segments=seg, factor=one, Fr=3, slot_of_row=None, n_dev=None)
        kw.update(over)
        with pytest.raises(ValueError, match=f"ctrl_warp_: .*{what}"):
            ctx.ctrl_warp_(**kw)
            pytest.fail(f"{over!r} was accepted")
    with pytest.raises(ValueError, match="4096"):
        ctx.ctrl_warp_(torch.zeros(1, 5000), [(0, 4097, 0)], torch.ones(1), 1)


# ---- the bank's host state ------------------------------------------------------------------------------------------------------
def _bank(model, n=3, **kw):
    import realtime
    return realtime.StreamBank(model, n, 44100, 0.1, 0.04, "cpu", buffer_num=4, use_graph=False, max_mix=3, **kw)


def test_bank_formant_row_and_refusals(lib_path):
    model = bank_model("CombSub", 4, 43)
    plain = _bank(model)
    assert plain.formant is None and plain._full.formant_term is None
    with pytest.raises(ValueError, match="without formant=True"):
        plain.set_formant(0, 1)
    with pytest.raises(ValueError, match="formant=True with models="):
        _bank(None, models=[model, model], formant=True)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="formant must be True or False"):
            _bank(model, formant=bad)
    bank = _bank(model, formant=True, active_widths=(1, 2), glide_breakpoints=3, pitch_breakpoints=2)
    assert bank.formant.tolist() == [1.0, 1.0, 1.0] and bank.formant.dtype == torch.float32 and bank._full.formant_term is bank.formant
    for W, rows in sorted(bank._compact.items()):
        assert rows.formant_term[0] is bank.formant and rows.formant_term[1] is rows.rows
    bank.set_formant(1, 4)
    bank.set_formant(2, -24)
    assert bank.formant.tolist() == [1.0, float(FC.factor(4)), 0.25] and bank.graph_builds == 0
    for slot, s in ((3, 1), (-1, 1), (True, 1), (0, 24.5), (0, float("nan")), (0, float("inf")), (0, "1")):
        with pytest.raises(ValueError):
            bank.set_formant(slot, s)
    assert bank.formant.tolist() == [1.0, float(FC.factor(4)), 0.25]                      # a refused call wrote nothing
    bank.reset(1)
    assert bank.formant.tolist() == [1.0, 1.0, 0.25]
