"""Key timelines, host side (no GPU): `infer_offline.KeyTimeline` and its refusals, `key_tables`, `job_table` with numeric keys
(unchanged) and with timelines, the `--jobs` entries of `main.py`, the two new symbols' place in the header, the library and the
ctypes table, the refusals of `StreamBank(pitch_breakpoints=)` and `set_pitch_timeline` - and the properties of the numpy
statement (tests/key_timeline_cases.py) that the GPU tests hold the kernels to."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import key_timeline_cases as KC
from conftest import ROOT
from test_bank_models_host import bank_model


# ---- KeyTimeline ----------------------------------------------------------------------------------------------------------------
def test_key_timeline_validation_and_frames():
    from infer_offline import KeyTimeline
    tl = KeyTimeline([(0, 0), (0.5, 2.0), [1.25, -3]])
    assert tl.points == [(0.0, 0.0), (0.5, 2.0), (1.25, -3.0)]
    assert tl.frames(44100, 512) == ([0, 43, 108], [0.0, 2.0, -3.0])             # int(round(t * sr / block))
    assert KeyTimeline([(0.2, 3.0)]).frames(44100, 512) == ([17], [3.0])
    assert KeyTimeline([(0.1, 1), (0.1, 1)]).points[1] == (0.1, 1.0)              # equal times are ascending; frames refuses them
    bad = [None, [], (), "x", [(0, 1, 2)], [3.0], [(-0.1, 0)], [(float("nan"), 0)], [(float("inf"), 0)], [(True, 0)], [("0", 0)],
           [(0.5, 0), (0.4, 0)], [(0, float("nan"))], [(0, float("inf"))], [(0, "2")], [(0, None)], [(0, True)], [(0, {1: 1.0})]]
    for points in bad:
        with pytest.raises(ValueError, match="KeyTimeline"):
            KeyTimeline(points)
            pytest.fail(f"{points!r} was accepted")
    for points in ([(0.100, 0), (0.101, 2)], [(0.1, 0), (0.1, 2)]):              # 0.1 s and 0.101 s both round to frame 9
        with pytest.raises(ValueError, match="both land on frame 9"):
            KeyTimeline(points).frames(44100, 512)


def test_key_tables_layout():
    from infer_offline import KeyTimeline, key_tables
    keys = [3.0, KeyTimeline([(0.2, 0), (1.0, 2.0)]), -12, KeyTimeline([(0.0, 0.1)]), 0]
    off, frame, semi, fac = key_tables(keys, 44100, 512)
    assert (off.dtype, frame.dtype, semi.dtype, fac.dtype) == (torch.int32, torch.int32, torch.float32, torch.float32)
    assert off.tolist() == [0, 1, 3, 4, 5, 6] and frame.tolist() == [0, 17, 86, 0, 0, 0]
    assert semi.tolist() == [3.0, 0.0, 2.0, -12.0, float(np.float32(0.1)), 0.0]
    # the factor is formed from the key as given (a Python float), not from its fp32 copy: `job_table`'s key_factor, stored to fp32
    want = torch.tensor([2 ** (k / 12) for k in (3.0, 0.0, 2.0, -12.0, 0.1, 0.0)], dtype=torch.float32)
    assert torch.equal(fac, want) and fac[3].item() == 0.5 and fac[1].item() == 1.0
    # the statement's own table builder agrees with it
    for got, ref in zip((off, frame, semi, fac), KC.tables([3.0, [(17, 0), (86, 2.0)], -12, [(0, 0.1)], 0])):
        assert np.array_equal(got.numpy(), ref)
    with pytest.raises(ValueError, match="both land on frame"):
        key_tables([KeyTimeline([(0.1, 0), (0.101, 1)])], 44100, 512)


# ---- job_table ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(lib_path):
    return [bank_model("CombSub", 2, 43), bank_model("Sins", 2, 44)]


PIECES = [(0, 0, 43, 0, 22016), (0, 77, 35, 39424, 17920), (1, 0, 60, 0, 30720)]


def test_job_table_is_unchanged_for_numbers_and_carries_timelines(models):
    from infer_offline import KeyTimeline, job_table
    numeric = [(0, 0, 1, 0), (0, 1, {1: 0.25, 2: 0.75}, 3), (1, 0, 2, -2.5)]
    table = job_table(PIECES, 2, numeric, models)
    assert table["key_factor"] == [1.0, 2 ** (3.0 / 12), 2 ** (-2.5 / 12)]
    assert table["model_of_job"] == [0, 1, 0] and table["speakers"] == [1, {1: 0.25, 2: 0.75}, 2]
    assert table["rows"] == [PIECES[0] + (0,), PIECES[1] + (0,), PIECES[0] + (1,), PIECES[1] + (1,), PIECES[2] + (2,)]
    assert table["piece_of_row"] == [0, 1, 0, 1, 2] and table["starts_per_job"] == [[0, 77], [0, 77], [0]]
    assert table["keys"] == [0.0, 3.0, -2.5] and all(isinstance(k, float) for k in table["keys"])
    tl = KeyTimeline([(0.0, 0), (1.0, 2)])
    timed = job_table(PIECES, 2, [numeric[0], (0, 1, 1, tl), numeric[2]], models)
    assert timed["keys"][1] is tl and timed["key_factor"] == [1.0, None, 2 ** (-2.5 / 12)]
    for name in ("rows", "piece_of_row", "starts_per_job", "model_of_job"):
        assert timed[name] == table[name], name
    with pytest.raises(ValueError, match="job 1: KeyTimeline: points 0 and 1 .* both land on frame 9"):
        job_table(PIECES, 2, [numeric[0], (0, 1, 1, KeyTimeline([(0.100, 0), (0.101, 2)]))], models)
    for key in ("3", None, [(0, 1)]):
        with pytest.raises(ValueError, match="job 0: key must be"):
            job_table(PIECES, 2, [(0, 0, 1, key)], models)


# ---- main.py --jobs -------------------------------------------------------------------------------------------------------------
def test_jobs_entries_take_a_key_timeline():
    import main
    from infer_offline import KeyTimeline, SpeakerTimeline
    spk, key = main._job_entry(0, {"id": 2, "key": 3, "suffix": "a"})
    assert spk == 2 and key == 3.0 and isinstance(key, float)
    assert main._job_entry(1, {"suffix": "b"}) == (1, 0.0)
    spk, key = main._job_entry(2, {"mix": {1: 0.5, 2: 0.5}, "key_timeline": [{"at": 0, "key": 0}, {"at": 1.5, "key": 2}], "suffix": "c"})
    assert spk == {1: 0.5, 2: 0.5} and isinstance(key, KeyTimeline) and key.points == [(0.0, 0.0), (1.5, 2.0)]
    spk, key = main._job_entry(3, {"timeline": [{"at": 0, "id": 1}, {"at": 1, "id": 2}], "key_timeline": [{"at": 0.5, "key": -1}],
                                   "suffix": "d"})
    assert isinstance(spk, SpeakerTimeline) and key.points == [(0.5, -1.0)]
    with pytest.raises(ValueError, match="entry 4 takes .* key or key_timeline"):       # both: like id with mix
        main._job_entry(4, {"key": 1, "key_timeline": [{"at": 0, "key": 1}], "suffix": "e"})
    with pytest.raises(ValueError, match="entry 5 takes"):
        main._job_entry(5, {"id": 1, "mix": {1: 1.0}, "suffix": "f"})
    with pytest.raises(ValueError, match="entry 6 takes"):
        main._job_entry(6, {"key_timeline": [{"at": 0, "key": 1}]})                     # no suffix
    for points in ([], {"at": 0, "key": 1}, [{"at": 0}], [{"at": 0, "key": 1, "id": 2}], [(0, 1)], None):
        with pytest.raises(ValueError, match="entry 7: key_timeline is a non-empty list"):
            main._job_entry(7, {"key_timeline": points, "suffix": "g"})
    with pytest.raises(ValueError, match="KeyTimeline: point 1: times must ascend"):
        main._job_entry(8, {"key_timeline": [{"at": 1, "key": 0}, {"at": 0.5, "key": 1}], "suffix": "h"})


# ---- symbols --------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_bound_and_exported(lib_path):
    import inspect

    import hipddsp
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddsp_amd.h")).read(), flags=re.S)
    declared = re.findall(r"\b(ddsp_\w+)\s*\(", text)
    lib = ctypes.CDLL(lib_path)
    for name, n_args in (("ddsp_pieces_gather_keys", 23), ("ddsp_bank_key_glide", 17)):
        assert declared.count(name) == 1 and name in hipddsp.SIGNATURES and hasattr(lib, name), name
        proto = re.search(rf"int {name}\((.*?)\);", text, flags=re.S).group(1)
        assert len(proto.split(",")) == len(hipddsp.SIGNATURES[name][1]) == n_args, name
    assert hipddsp.SIGNATURES["ddsp_bank_key_glide"][1][15] is ctypes.c_double
    for name in ("ddsp_pieces_gather", "ddsp_pieces_gather_jobs", "ddsp_bank_glide", "ddsp_mix_timeline"):
        assert hasattr(lib, name), name
    assert "key_timeline" in inspect.signature(hipddsp.Context.pieces_gather).parameters
    assert inspect.signature(hipddsp.Context.pieces_gather).parameters["key_timeline"].default is None
    assert hasattr(hipddsp.Context, "bank_key_glide_")
    assert hipddsp.ABI_VERSION == 8 and lib.ddsp_abi_version() == 8


# ---- the statement --------------------------------------------------------------------------------------------------------------
def test_statement_is_exact_at_breakpoints_constant_on_equal_semitones_and_monotone_on_a_slope():
    times = [10, 20, 30, 50]
    semi = np.array([0.0, 3.0, 3.0, -1.5], dtype=np.float32)
    fac = np.array([KC.stored_factor(k) for k in semi])
    taus = np.arange(0, 61, dtype=np.float64)
    got, stored = KC.factors(times, semi, fac, taus)
    assert got.dtype == np.float32
    assert np.array_equal(got[:11], np.full(11, fac[0])) and stored[:11].all()              # (a), and (c) at 10
    assert np.array_equal(got[20:31], np.full(11, fac[1])) and stored[20:31].all()          # (c) at 20, (d) up to 29, (c) at 30
    assert got[30] == fac[2] and got[50] == fac[3] and np.array_equal(got[50:], np.full(11, fac[3])) and stored[50:].all()
    assert not stored[11:20].any() and not stored[31:50].any()
    assert (np.diff(got[10:21]) > 0).all() and (np.diff(got[30:51]) < 0).all()               # monotone on the slopes
    assert got[15] == np.float32(2.0 ** (1.5 / 12)) and got[40] == np.float32(2.0 ** (0.75 / 12))
    # fractional times (a bank's frames at a fractional hop) between and on the breakpoints
    got, stored = KC.factors(times, semi, fac, [9.999, 10.0, 10.001, 49.999, 50.0])
    assert stored.tolist() == [True, True, False, False, True] and fac[0] < got[2] < np.float32(2.0 ** (0.01 / 12))
    # one breakpoint: the stored factor everywhere, which is the host's factor of the constant key
    got, stored = KC.factors([7], [np.float32(0.1)], [KC.stored_factor(0.1)], taus)
    assert stored.all() and np.array_equal(got, np.full(61, np.float32(2 ** (0.1 / 12))))
    assert KC.stored_factor(3.0) == torch.tensor(2 ** (3.0 / 12), dtype=torch.float32).item()


def test_statement_of_the_bank_kernel_clocks_and_padding():
    S, P = 3, 4
    z = dict(clock=np.array([100, 7, 2 ** 40], dtype=np.int64), key_n=np.array([0, 2, 2], dtype=np.int32),
             key_t=np.zeros((S, P), dtype=np.int64), key_semi=np.zeros((S, P), dtype=np.float32),
             key_fac=np.ones((S, P), dtype=np.float32), pitch=np.array([1.5, 0.75, 1.25], dtype=np.float32))
    z["key_t"][2, :2] = [2 ** 40, 2 ** 40 + 9600]
    z["key_semi"][2, :2] = [0, 2]
    z["key_fac"][2, :2] = [1.0, KC.stored_factor(2)]
    got, stored, clock = KC.bank_pitch_frames([2, -1, 0, 3], 4, **z, Fr=21, n_in=9600, block=9600, hop=557.28)
    assert clock.tolist() == [100 + 9600, 7, 2 ** 40 + 9600]                                  # slot 1 is not named
    assert np.array_equal(got[1], np.ones(21, dtype=np.float32)) and np.array_equal(got[3], np.ones(21, dtype=np.float32))
    assert np.array_equal(got[2], np.full(21, np.float32(1.5))) and stored[1:].all()
    # slot 2: frame 0 sits on the first breakpoint, frames 1..17 on the slope, frames 18.. (18 * 557.28 > 9600) behind the last
    assert got[0, 0] == 1.0 and stored[0, 0] and not stored[0, 1:18].any() and stored[0, 18:].all()
    assert (np.diff(got[0, :19]) > 0).all() and np.array_equal(got[0, 18:], np.full(3, KC.stored_factor(2)))


# ---- the bank's refusals --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(lib_path):
    return bank_model("CombSub", 4, 43)


def _bank(model, n=3, **kw):
    import realtime
    return realtime.StreamBank(model, n, 44100, 0.1, 0.04, "cpu", buffer_num=4, use_graph=False, max_mix=3, **kw)


def test_pitch_breakpoints_state_and_refusals(model):
    from infer_offline import KeyTimeline, SpeakerTimeline
    plain = _bank(model)
    assert plain.pitch_breakpoints is None and plain._full.pitch_frames is None and plain._full.pitch_term is plain.pitch
    assert all(getattr(plain, name) is None for name in ("key_clock", "key_n", "key_t", "key_semi", "key_fac", "last_pitch"))
    for bad in (0, 65, -1, True, 4.0, "4", (4,)):
        with pytest.raises(ValueError, match="pitch_breakpoints"):
            _bank(model, pitch_breakpoints=bad)
            pytest.fail(f"{bad!r} was accepted")
    # independent of glide_breakpoints, and allowed with models= and active_widths=
    bank = _bank(None, models=[model, model], pitch_breakpoints=4, active_widths=(1, 2))
    assert bank.glide_clock is None and bank.key_t.shape == (3, 4)
    both = _bank(model, pitch_breakpoints=2, glide_breakpoints=5)
    assert both.key_t.shape == (3, 2) and both.glide_t.shape == (3, 5)
    assert (bank.key_clock.dtype, bank.key_n.dtype, bank.key_t.dtype, bank.key_semi.dtype, bank.key_fac.dtype) == \
        (torch.int64, torch.int32, torch.int64, torch.float32, torch.float32)
    assert bank.key_clock.shape == (3,) and bank.key_n.shape == (3,) and bank.key_semi.shape == bank.key_fac.shape == (3, 4)
    for W, rows in [(3, bank._full)] + sorted(bank._compact.items()):
        assert rows.pitch_frames.shape == (W, bank.frames) and rows.pitch_term is rows.pitch_frames and rows.w_frames is None
    tl = KeyTimeline([(0.0, 0), (0.25, 2), (0.5, -1)])
    with pytest.raises(ValueError, match="without pitch_breakpoints"):
        plain.set_pitch_timeline(0, tl)
    bank.set_pitch(1, 5)
    bank.set_pitch_timeline(1, tl, at=0.1)
    assert int(bank.key_n[1]) == 3 and int(bank.key_clock[1]) == 4410 and bank.key_t[1].tolist() == [0, 11025, 22050, 0]
    assert bank.key_semi[1].tolist() == [0.0, 2.0, -1.0, 0.0]
    assert torch.equal(bank.key_fac[1], torch.tensor([1.0, 2 ** (2.0 / 12), 2 ** (-1.0 / 12), 1.0], dtype=torch.float32))
    assert not bank.key_n[[0, 2]].any() and not bank.key_clock[[0, 2]].any() and bank.graph_builds == 0
    names = ("pitch", "key_clock", "key_n", "key_t", "key_semi", "key_fac")
    state = [getattr(bank, name).clone() for name in names]
    bad = [(1, KeyTimeline([(0.0, 0), (0.1, 1), (0.2, 0), (0.3, 1), (0.4, 0)]), "pitch_breakpoints = 4"),
           (1, KeyTimeline([(0.100000, 0), (0.100004, 2)]), "both land on sample 4410"),
           (3, tl, "slot"), (-1, tl, "slot"), (True, tl, "slot"),
           (1, [(0.0, 1)], "KeyTimeline"), (1, SpeakerTimeline([(0.0, 1)]), "KeyTimeline")]
    for slot, timeline, match in bad:
        with pytest.raises(ValueError, match=match):
            bank.set_pitch_timeline(slot, timeline)
            pytest.fail(f"{match!r} was accepted")
    for at in (float("nan"), float("inf"), "0", None, True):
        with pytest.raises(ValueError, match="at must be"):
            bank.set_pitch_timeline(1, tl, at=at)
    for name, want in zip(names, state):
        assert torch.equal(getattr(bank, name), want), name                          # a refused call wrote nothing
    # set_pitch ends the timeline and keeps the clock; reset zeroes the clock and keeps the timeline
    bank.set_pitch_timeline(2, tl)
    bank.set_pitch(1, 3)
    assert int(bank.key_n[1]) == 0 and int(bank.key_clock[1]) == 4410
    assert bank.pitch[1].item() == torch.tensor(2 ** (3.0 / 12), dtype=torch.float32).item()
    bank.key_clock[2] = 999
    bank.reset(2)
    assert int(bank.key_clock[2]) == 0 and int(bank.key_n[2]) == 3 and bank.key_t[2].tolist() == [0, 11025, 22050, 0]
    assert int(bank.key_clock[1]) == 4410
