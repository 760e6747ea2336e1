"""A speaker mix per FRAME, host side (no GPU): `infer_offline.SpeakerTimeline`, `job_table` with timelines, the tables of
`ddsp_mix_timeline`, the refusals of `hipddsp.check_mix_frames` and of the tensor-valued `spk_mix_dict`, the two new symbols'
place in the header and the ctypes table - and the numpy statement of `ddsp_mix_timeline` that the GPU test holds the kernel to."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from infer_offline import SpeakerTimeline, job_table, piece_table, timeline_tables
from test_bank_models_host import bank_model

BLOCK, SR = 512, 44100
SLICES = [[(0, 20 * BLOCK), (30 * BLOCK, 57 * BLOCK)], [(BLOCK, 31 * BLOCK)]]


def timeline_weights(rows, J, bp_off, bp_frame, bp_w, job_ids, N_max):
    """The numpy statement of `ddsp_mix_timeline` (include/ddsp_amd.h) -> (ids (R, K) int32, w (R, N_max, K) fp32).  rows: (R, 6)
    (file, start_frame, n_frames, start_sample, n_samples, job).  Frame t < n_frames of row r is file frame f = start_frame + t;
    its weights are the job's breakpoints interpolated at f in fp64, w0 + (w1 - w0) * ((f - f0) / (f1 - f0)), rounded to fp32;
    constant before the first and after the last breakpoint; exact zeros for t >= n_frames; a job outside [0, J) is a padding
    row, ids 1 and weights 0."""
    rows, bp_off, bp_frame = np.asarray(rows, dtype=np.int64).reshape(-1, 6), np.asarray(bp_off), np.asarray(bp_frame)
    bp_w, job_ids = np.asarray(bp_w, dtype=np.float32), np.asarray(job_ids, dtype=np.int32)
    K = job_ids.shape[1]
    ids = np.ones((len(rows), K), dtype=np.int32)
    w = np.zeros((len(rows), int(N_max), K), dtype=np.float32)
    for r, (_, start, n, _, _, job) in enumerate(rows):
        if not 0 <= job < J or bp_off[job + 1] <= bp_off[job]:
            continue
        ids[r] = job_ids[job]
        lo, hi = int(bp_off[job]), int(bp_off[job + 1])
        at = bp_frame[lo:hi]
        for t in range(min(int(n), int(N_max))):
            f = start + t
            p = lo + int(np.searchsorted(at, f, side="right"))      # the first breakpoint behind f
            if p == lo:
                w[r, t] = bp_w[lo]
            elif p == hi:
                w[r, t] = bp_w[hi - 1]
            else:
                w0, w1 = bp_w[p - 1].astype(np.float64), bp_w[p].astype(np.float64)
                frac = np.float64(f - bp_frame[p - 1]) / np.float64(bp_frame[p] - bp_frame[p - 1])
                w[r, t] = (w0 + (w1 - w0) * frac).astype(np.float32)
    return ids, w


@pytest.fixture(scope="module")
def models(lib_path):
    return [bank_model("CombSub", 4, 43), bank_model("Sins", 2, 44)]


def test_timeline_rounds_seconds_to_frames():
    tl = SpeakerTimeline([(0, 1), (0.5, {2: 0.25, 1: 0.75}), (1.0, 3)])
    assert tl.ids == [1, 2, 3]                                        # first appearance
    at, w = tl.frames(SR, BLOCK)
    assert at == [0, int(round(0.5 * SR / BLOCK)), int(round(1.0 * SR / BLOCK))] == [0, 43, 86]
    assert w == [[1.0, 0.0, 0.0], [0.75, 0.25, 0.0], [0.0, 0.0, 1.0]]  # an id a point does not name weighs 0 there; not normalised
    # Python's round: half to even on the exact product (t = 1.5 frames -> 2, t = 2.5 frames -> 2 would collide with it)
    assert SpeakerTimeline([(1.5 * BLOCK / SR, 1)]).frames(SR, BLOCK)[0] == [int(round(1.5 * BLOCK / SR * SR / BLOCK))]
    assert SpeakerTimeline([(0.011, 1)]).frames(SR, BLOCK)[0] == [1] and SpeakerTimeline([(0.0174, 1)]).frames(SR, BLOCK)[0] == [1]
    assert SpeakerTimeline([(0.0175, 1)]).frames(SR, BLOCK)[0] == [2]
    assert SpeakerTimeline([(0.0, {2: 3.0, 1: -1.0})]).frames(SR, BLOCK) == ([0], [[3.0, -1.0]])


def test_timeline_refusals():
    for bad in ([], None, [(0.0,)], [(-0.1, 1)], [(float("nan"), 1)], [(float("inf"), 1)], [(1.0, 1), (0.5, 2)], [(0.0, 0)],
                [(0.0, {})], [(0.0, {1.5: 1.0})], [(0.0, "1")], [("0", 1)], [(0.0, {1: "x"})], [(True, 1)]):
        with pytest.raises(ValueError, match="SpeakerTimeline"):
            SpeakerTimeline(bad)
    with pytest.raises(ValueError, match="at most 16 distinct ids"):
        SpeakerTimeline([(0.0, {i: 1.0 for i in range(1, 10)}), (1.0, {i: 1.0 for i in range(9, 18)})])
    SpeakerTimeline([(0.0, {i: 1.0 for i in range(1, 17)})])        # 16 ids are fine
    two = SpeakerTimeline([(0.100, 1), (0.104, 2)])                 # 8.61 and 8.96 frames: both frame 9
    with pytest.raises(ValueError, match="both land on frame 9"):
        two.frames(SR, BLOCK)
    assert two.frames(SR, 128)[0] == [34, 36]                       # (a finer frame rate keeps them apart)
    with pytest.raises(ValueError, match="both land on frame"):
        SpeakerTimeline([(0.5, 1), (0.5, 2)]).frames(SR, BLOCK)


def test_job_table_with_timelines(models):
    pieces = piece_table(SLICES, float(BLOCK))
    plain = [(0, 0, 1, 0), (1, 1, {1: 0.25, 2: 0.75}, 3), (0, 1, 2, -1)]
    want = job_table(pieces, 2, plain, models)
    tl = SpeakerTimeline([(0.0, 1), (0.4, {4: 1.0})])
    got = job_table(pieces, 2, plain + [(1, 0, tl, 2)], models)
    # the id and dict jobs get the tables they always got; the timeline stands in `speakers` as it is
    for key in want:
        assert got[key][:len(want[key])] == want[key], key
    assert set(got) == set(want) and got["speakers"][3] is tl and got["model_of_job"][3] == 0
    assert [row[5] for row in got["rows"]][-1] == 3 and got["key_factor"][3] == 2 ** (2 / 12)
    # ids are held to the JOB's model: 4 is a speaker of model 0 and none of model 1 (n_spk = 2)
    with pytest.raises(ValueError, match=r"job 0: speaker id 4 is outside \[1, 2\] of models\[1\]"):
        job_table(pieces, 2, [(0, 1, tl, 0)], models)
    with pytest.raises(ValueError, match="job 1: SpeakerTimeline: points 0 and 1"):
        job_table(pieces, 2, [(0, 0, 1, 0), (0, 0, SpeakerTimeline([(0.100, 1), (0.104, 2)]), 0)], models)
    with pytest.raises(ValueError, match="at most 16 distinct ids"):            # too many ids never reach a table
        job_table(pieces, 2, [(0, 0, SpeakerTimeline([(0.0, {i: 1.0 for i in range(1, 18)})]), 0)], models)
    # every refusal of today stays, the one for an spk that is neither an id nor a dict (nor a timeline) among them
    with pytest.raises(ValueError, match="spk must be a speaker id or a mix dict"):
        job_table(pieces, 2, [(0, 0, "1", 0)], models)
    with pytest.raises(ValueError, match="a speaker mix holds 1 to 16 ids"):
        job_table(pieces, 2, [(0, 0, {}, 0)], models)
    with pytest.raises(ValueError, match=r"speaker id 5 is outside \[1, 4\] of models\[0\]"):
        job_table(pieces, 2, [(0, 0, 5, 0)], models)


def test_timeline_tables_make_ids_and_dicts_one_breakpoint():
    tl = SpeakerTimeline([(0.0, 1), (0.5, {3: 0.5, 1: 0.5}), (1.0, 3)])
    speakers = [2, tl, {4: 0.25, 1: 0.75}, 7]
    off, frame, w, ids = timeline_tables(speakers, [0, 1, 2], SR, BLOCK)      # job 3 belongs to another model
    assert (off.dtype, frame.dtype, w.dtype, ids.dtype) == (torch.int32, torch.int32, torch.float32, torch.int32)
    assert off.tolist() == [0, 1, 4, 5, 5] and frame.tolist() == [0, 0, 43, 86, 0]
    assert ids.tolist() == [[2, 1], [1, 3], [4, 1], [1, 1]]                   # short rows padded with id 1 ...
    assert w.tolist() == [[1.0, 0.0], [1.0, 0.0], [0.5, 0.5], [0.0, 1.0], [0.25, 0.75]]        # ... and weight 0
    # through the numpy statement: a constant mix for the id and the dict, a padding row for the job without breakpoints
    rows = [(0, 5, 4, 0, 0, 0), (0, 40, 6, 0, 0, 1), (1, 0, 3, 0, 0, 2), (1, 0, 3, 0, 0, 3)]
    got_ids, got_w = timeline_weights(rows, 4, off.numpy(), frame.numpy(), w.numpy(), ids.numpy(), 6)
    assert got_ids.tolist() == [[2, 1], [1, 3], [4, 1], [1, 1]]
    assert np.array_equal(got_w[0], np.array([[1, 0]] * 4 + [[0, 0]] * 2, dtype=np.float32))
    assert np.array_equal(got_w[2], np.array([[0.25, 0.75]] * 3 + [[0, 0]] * 3, dtype=np.float32)) and not got_w[3].any()
    assert got_w[1, 3].tolist() == [0.5, 0.5]                                 # frame 43: exactly the breakpoint
    assert got_w[1, 0, 0] == np.float32(1.0 + (0.5 - 1.0) * (40 / 43)) and got_w[1, 4, 1] == np.float32(0.5 + 0.5 * (1 / 43))


def test_check_mix_frames_refusals():
    import hipddsp
    B, Fr, K = 3, 5, 2
    ids, w = torch.ones(B, K, dtype=torch.int32), torch.zeros(B, Fr, K)
    assert hipddsp.check_mix_frames(ids, w, B, Fr) == K
    assert hipddsp.check_mix_frames(torch.ones(B, 16, dtype=torch.int32), torch.zeros(B, Fr, 16), B, Fr) == 16
    for bad_ids, bad_w in [(ids.long(), w), (ids, w.double()), (ids, w[:, :, 0]), (ids, torch.zeros(B, K)), (ids[:2], w),
                           (ids, torch.zeros(B, Fr + 1, K)), (ids, torch.zeros(B, Fr, K + 1)), (ids.reshape(-1), w),
                           (torch.ones(B, 0, dtype=torch.int32), torch.zeros(B, Fr, 0)),
                           (torch.ones(B, 17, dtype=torch.int32), torch.zeros(B, Fr, 17)),
                           (ids, torch.zeros(B, K, Fr).transpose(1, 2)), (ids.t().contiguous().t(), w), (ids.numpy(), w), (ids, None)]:
        with pytest.raises(ValueError, match="frame mix"):
            hipddsp.check_mix_frames(bad_ids, bad_w, B, Fr)
    with pytest.raises(ValueError, match="one device"):
        hipddsp.check_mix_frames(ids, w.to("meta"), B, Fr)


def test_tensor_valued_mix_dict_becomes_the_frame_form():
    from ddsp.unit2control import is_frame_mix, mix_frames_of_dict
    B, Fr = 2, 5
    ramp = torch.linspace(0, 1, Fr)
    assert mix_frames_of_dict(None, B, Fr, "cpu", 8) is None
    assert mix_frames_of_dict({1: 0.5, 2: 0.5}, B, Fr, "cpu", 8) is None                  # numbers only: the host mix, as ever
    assert mix_frames_of_dict({1: torch.tensor(0.5)}, B, Fr, "cpu", 8) is None            # (a 0-d tensor is a number)
    full = torch.arange(B * Fr, dtype=torch.float32).reshape(B, Fr, 1)
    ids, w = mix_frames_of_dict({7: full, 2: ramp.reshape(1, Fr, 1), 3: ramp, 1: 0.25}, B, Fr, "cpu", 8)
    assert ids.dtype == torch.int32 and ids.tolist() == [[7, 2, 3, 1]] * B                # dict order
    assert w.dtype == torch.float32 and w.shape == (B, Fr, 4) and w.is_contiguous() and is_frame_mix((ids, w))
    assert torch.equal(w[:, :, 0], full[:, :, 0]) and torch.equal(w[1, :, 1], ramp) and torch.equal(w[0, :, 2], ramp)
    assert torch.equal(w[:, :, 3], torch.full((B, Fr), 0.25))
    assert not is_frame_mix((ids, w[:, 0])) and not is_frame_mix(None)
    for bad in ({1: torch.zeros(B, Fr + 1, 1)}, {1: torch.zeros(B + 1, Fr, 1)}, {1: torch.zeros(B, Fr, 2)}, {1: torch.zeros(Fr, 1)}):
        with pytest.raises(ValueError, match="per-frame weight"):
            mix_frames_of_dict(bad, B, Fr, "cpu", 8)
    with pytest.raises(ValueError, match=r"speaker id 9 is outside \[1, 8\]"):
        mix_frames_of_dict({9: ramp}, B, Fr, "cpu", 8)
    with pytest.raises(ValueError, match="1 to 16 ids"):
        mix_frames_of_dict({i: ramp for i in range(1, 18)}, B, Fr, "cpu", 32)


def test_frame_mix_is_inference_only(lib_path):
    """The per-frame form refuses a network that wants gradients as the row mix does, before anything is launched."""
    model = bank_model("CombSub", 4, 43)
    B, Fr = 1, 4
    pair = (torch.ones(B, 1, dtype=torch.int32), torch.ones(B, Fr, 1))
    u = model.unit2ctrl
    with pytest.raises(NotImplementedError, match="inference only"):
        u.frame_mix(None, pair, B, Fr, "cpu")
    with pytest.raises(NotImplementedError, match="inference only"):
        u.frame_mix({1: torch.ones(Fr)}, None, B, Fr, "cpu")
    with torch.no_grad():
        assert u.frame_mix(None, pair, B, Fr, "cpu") == (None, pair)
        assert u.frame_mix({1: 0.5}, None, B, Fr, "cpu") == ({1: 0.5}, None)                # untouched
        with pytest.raises(ValueError, match="mutually exclusive"):
            u.frame_mix({1: 0.5}, pair, B, Fr, "cpu")
        with pytest.raises(ValueError, match="mutually exclusive"):
            model._mix_keyword((pair[0], pair[1][:, 0]), {"spk_mix_frames": pair})
        with pytest.raises(ValueError, match="spk_mix_frames must be a pair"):
            model._mix_keyword(None, {"spk_mix_frames": (pair[0], pair[1][:, 0])})
        assert model._mix_keyword(None, {"spk_mix_frames": pair}) == pair and model._mix_keyword(None, {}) is None


def test_new_symbols_are_declared_bound_and_exported(lib_path):
    import hipddsp
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddsp_amd.h")).read(), flags=re.S)
    declared = re.findall(r"\b(ddsp_\w+)\s*\(", text)
    lib = ctypes.CDLL(lib_path)
    for name in ("ddsp_unit2ctrl_fwd_framemix", "ddsp_mix_timeline"):
        assert declared.count(name) == 1 and name in hipddsp.SIGNATURES and hasattr(lib, name), name
    # the per-frame call has the row mix's signature: the weights' shape is all that differs
    assert [a for a in hipddsp.SIGNATURES["ddsp_unit2ctrl_fwd_framemix"][1]] == \
        [a for a in hipddsp.SIGNATURES["ddsp_unit2ctrl_fwd_rowmix"][1]]
    proto = re.search(r"int ddsp_mix_timeline\((.*?)\);", text, flags=re.S).group(1)
    assert len(proto.split(",")) == len(hipddsp.SIGNATURES["ddsp_mix_timeline"][1]) == 14
    assert hasattr(hipddsp.Context, "unit2ctrl_framemix") and hasattr(hipddsp.Context, "mix_timeline")
    assert hipddsp.ABI_VERSION == 8
