"""The silence slicer on the host (no GPU): the numpy restatement of tests/slicer_cases.py against what the reference's own
`Slicer` returned (tests/golden/slicer_ref.npz), the condition on the cases, the three symbols, the frame count out of the
library, the capacity bound, the constructor's arithmetic and refusals, and `split`'s filter."""
import inspect
import os
import re

import numpy as np
import pytest

import slicer_cases as SC
from conftest import GOLDEN, ROOT

NEW = ["ddsp_slicer_frames", "ddsp_slicer"]


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "slicer_ref.npz"))


@pytest.fixture(scope="module")
def restated():
    """{(case, pad mode): the fp64 restatement's tagger dict} - computed once, with the condition on the cases asserted."""
    return {(name, mode): SC.check_conditions(name, mode) for name in SC.CASES for mode in SC.PAD_MODES}


def test_fixture_holds_the_cases_of_this_file(g):
    assert [str(n) for n in g["names"]] == list(SC.CASES) and tuple(str(m) for m in g["pad_modes"]) == SC.PAD_MODES
    for name, (pset, *_rest) in SC.CASES.items():
        x = SC.signal(name)
        fr = SC.frames_of(SC.PARAMS[pset])
        assert x.dtype == np.float32 and x.shape[0] == int(g[f"{name}_n"]) and x.shape[0] <= 20000
        # the seeded signal is the one the reference was run on
        assert np.isclose(np.sum(x.astype(np.float64) ** 2), float(g[f"{name}_energy"]), rtol=1e-12, atol=0)
        assert [fr[k] for k in ("hop", "win", "min_length", "min_interval", "max_sil_kept")] == g[f"{name}_frames"].tolist()
        assert fr["threshold"] == float(g[f"{name}_threshold"])
    wins = {SC.frames_of(p)["win"] for p in SC.PARAMS.values()}
    assert any(w % 2 for w in wins) and any(w % 80 and not w % 2 for w in wins)     # an odd window, one that is no multiple of the hop


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_equals_the_reference(g, dtype):
    for name in SC.CASES:
        for mode in SC.PAD_MODES:
            got = SC.restate(name, mode, dtype)[3]["chunks"]
            want = g[f"{name}_{mode}_chunks"]
            assert got.shape == want.shape and np.array_equal(got, want), (name, mode)
            assert SC.chunk_dict(got) == SC.chunk_dict(want)


def test_fp32_restatement_within_the_cap():
    worst = max(SC.rms_difference(SC.restate(name, mode, np.float32)[2], SC.restate(name, mode, np.float64)[2])
                for name in SC.CASES for mode in SC.PAD_MODES)
    print(f"frame RMS, fp32 against fp64 restatement: largest relative difference {worst:.3e}")
    assert SC.RMS_RTOL / 8 <= worst <= SC.RMS_RTOL / 4 * 1.01, worst        # the constant is 4 x this measurement


def test_cases_take_every_path(g, restated):
    seen = set().union(*(t["paths"] for t in restated.values()))
    assert seen == set(SC.ALL_PATHS), sorted(set(SC.ALL_PATHS) - seen)
    # from the reference run's line trace: the early return, the cleared run, the three placement branches each from frame 0
    # and from a later frame, the trailing tag, no tags, the leading voiced chunk and the closing chunk (slicer.py's lines)
    ran = set().union(*(set(g[f"{name}_{mode}_lines"].tolist()) for name in SC.CASES for mode in SC.PAD_MODES))
    assert {33, 52, 58, 60, 68, 71, 77, 79, 87, 90, 95, 107} <= ran
    # an argmin over exact zeros, where only the tie-break decides
    _, _, r, t = SC.restate("zeros", "constant")
    assert any(np.count_nonzero(r[lo:hi] == 0.0) > 1 for lo, hi in t["ranges"])
    # a zero-length silence chunk, a range clipped at the array's end
    assert any((t["chunks"][:, 0] == t["chunks"][:, 1]).any() for t in restated.values())
    for (name, mode), t in restated.items():
        fr = SC.frames_of(SC.PARAMS[SC.CASES[name][0]])
        n = int(SC.signal(name).shape[0])
        assert all(hi <= SC.n_frames(n, fr["win"], fr["hop"]) for _, hi in t["ranges"])


def test_reflect_padding_is_the_periodic_rule():
    """The index rule the kernel selects by (period 2 (n - 1)) is numpy's 'reflect', also where the padding is longer than the row."""
    for n, pad in ((1, 5), (2, 7), (3, 5), (50, 160), (80, 100)):
        x = np.arange(n, dtype=np.float64)
        y = np.pad(x, pad, mode="reflect")
        p = 2 * (n - 1)
        for k in range(y.shape[0]):
            j = k - pad
            m = 0 if n == 1 else j % p
            assert y[k] == x[m if m < n else p - m], (n, pad, k)


def test_symbols_are_declared_exported_and_bound(lib_path):
    import hipddsp
    lib = hipddsp.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddsp_amd.h")).read(), flags=re.S)
    for name in NEW:
        assert name in hipddsp.SIGNATURES, name
        assert getattr(lib, name).argtypes == hipddsp.SIGNATURES[name][1]
        decl = re.search(r"\bint(?:64_t)? " + name + r"\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in include/ddsp_amd.h"
        assert len(decl.group(1).split(",")) == len(hipddsp.SIGNATURES[name][1]), name
    assert hipddsp.ABI_VERSION == 8 and lib.ddsp_abi_version() == 8
    # one binding method: the ragged form is an argument of it
    assert inspect.signature(hipddsp.Context.slicer).parameters["n_dev"].default is None
    assert not hasattr(hipddsp.Context, "slicer_ragged")


def test_frame_count_out_of_the_library(lib_path):
    import hipddsp
    for win, hop in ((320, 80), (200, 80), (201, 80), (3528, 882), (1, 1), (7, 3)):
        for n in (0, 1, 2, hop - 1, hop, hop + 1, win - 1, win, win + 1, 10 * hop + 3, 20000):
            if n + 2 * (win // 2) < win:
                assert hipddsp.load_library().ddsp_slicer_frames(n, win, hop) == -1
                continue
            want = SC.n_frames(n, win, hop)
            assert hipddsp.slicer_frames(n, win, hop) == want, (n, win, hop)
            if n >= 1:
                assert want == SC.rms(np.zeros(n), win, hop).shape[0]
    for bad in ((-1, 4, 2), (5, 0, 2), (5, 4, 0)):
        with pytest.raises(ValueError):
            hipddsp.slicer_frames(*bad)


def test_capacity_bound_holds(lib_path, restated):
    import hipddsp
    for (name, mode), t in restated.items():
        fr = SC.frames_of(SC.PARAMS[SC.CASES[name][0]])
        F = SC.n_frames(int(SC.signal(name).shape[0]), fr["win"], fr["hop"])
        cap = hipddsp.slicer_capacity(F, fr["min_interval"])
        assert cap == SC.capacity(F, fr["min_interval"])
        assert len(t["tags"]) <= F // fr["min_interval"] + 1 and t["chunks"].shape[0] <= 2 * max(len(t["tags"]), 0) + 1 <= cap
    # the densest tagging there is: silent runs of exactly min_interval frames, one voiced frame between them
    fr = dict(hop=1, win=1, threshold=0.5, min_length=1, min_interval=2, max_sil_kept=1)
    r = np.tile([0.0, 0.0, 1.0], 40)[:-1]
    t = SC.tag(r, r.shape[0], fr)
    assert len(t["tags"]) == 40 and t["chunks"].shape[0] <= hipddsp.slicer_capacity(r.shape[0], 2)
    with pytest.raises(ValueError):
        hipddsp.slicer_capacity(10, 0)


def test_constructor_arithmetic_and_refusals(g):
    from slicer import Slicer
    for name, (pset, *_rest) in SC.CASES.items():
        s = Slicer(**SC.PARAMS[pset])
        assert [s.hop_size, s.win_size, s.min_length, s.min_interval, s.max_sil_kept] == g[f"{name}_frames"].tolist()
        assert s.threshold == float(g[f"{name}_threshold"])
    s = Slicer(44100)
    assert (s.hop_size, s.win_size, s.min_length, s.min_interval, s.max_sil_kept) == (882, 3528, 250, 15, 250)
    assert s.pad_mode == "constant"
    assert list(inspect.signature(Slicer.__init__).parameters)[1:] == ["sr", "threshold", "min_length", "min_interval", "hop_size",
                                                                       "max_sil_kept", "pad_mode", "device"]
    with pytest.raises(ValueError, match=r"^The following condition must be satisfied: min_length >= min_interval >= hop_size$"):
        Slicer(8000, min_length=100, min_interval=300)
    with pytest.raises(ValueError, match=r"^The following condition must be satisfied: min_length >= min_interval >= hop_size$"):
        Slicer(8000, min_interval=10, hop_size=20)
    with pytest.raises(ValueError, match=r"^The following condition must be satisfied: max_sil_kept >= hop_size$"):
        Slicer(8000, max_sil_kept=10)
    with pytest.raises(ValueError, match="pad_mode"):
        Slicer(8000, pad_mode="edge")


def test_two_dimensional_input_is_refused():
    import torch
    from slicer import Slicer, cut
    s = Slicer(8000)
    for stereo in (np.zeros((2, 4000), dtype=np.float32), torch.zeros(2, 4000)):
        with pytest.raises(ValueError, match="mono"):
            s.slice(stereo)
        with pytest.raises(ValueError, match="mono"):
            s.chunk_rows(stereo)
    with pytest.raises(ValueError, match="mono"):
        cut(np.zeros((2, 4000), dtype=np.float32), 8000)
    assert list(inspect.signature(cut).parameters) == ["audio", "sr", "db_thresh", "min_len"]
    assert inspect.signature(cut).parameters["db_thresh"].default == -30
    # an empty file is the reference's early return
    assert s.slice(np.zeros(0, dtype=np.float32)) == {"0": {"slice": False, "split_time": "0,0"}}


def test_counts_go_through_the_slicer_rule(lib_path):
    import hipddsp
    assert hipddsp.check_n_samples([1, 5], 2, 5, hipddsp.slicer_rule) == [1, 5]
    with pytest.raises(ValueError, match=r"n_samples\[1\] = 0"):
        hipddsp.check_n_samples([3, 0], 2, 5, hipddsp.slicer_rule)
    assert hipddsp.slicer_rule(1) is None and "at least 1" in hipddsp.slicer_rule(0)


def test_split_drops_zero_length_chunks_and_keeps_silence(g, monkeypatch):
    import infer_offline
    import slicer
    rows = g["all_b_constant_chunks"]
    assert (rows[:, 0] == rows[:, 1]).any() and (rows[:, 2] == 1).any()
    seen = {}

    def chunk_rows(self, waveform):
        seen["args"] = (self.hop_size, self.min_length, self.threshold)
        return rows.astype(np.int32)
    monkeypatch.setattr(slicer.Slicer, "chunk_rows", chunk_rows)
    got = infer_offline.split(np.zeros(8), 8000, 80.0)
    assert got == [(int(a), int(b)) for a, b, _ in rows if a != b] and len(got) < len(rows)
    assert any(s == 1 and a != b and (int(a), int(b)) in got for a, b, s in rows)          # a silence chunk is kept
    assert all(isinstance(v, int) for pair in got for v in pair)
    assert seen["args"] == (160, 250, 10 ** (-40 / 20.))                                   # main.split's defaults: -40 dB, 5000 ms
    p = inspect.signature(infer_offline.split).parameters
    assert list(p) == ["audio", "sample_rate", "hop_size", "db_thresh", "min_len"]
    assert (p["db_thresh"].default, p["min_len"].default) == (-40, 5000)
