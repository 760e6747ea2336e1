"""The speaker glide of `realtime.StreamBank(glide_breakpoints=...)`, host side (no GPU): `glide_ref`, the numpy statement of
`ddsp_bank_glide` that the GPU test holds the kernel to, and its properties; the new symbol's place in the header, the library
and the ctypes table; the refusals of the constructor and of `set_timeline`, all raised before anything needs a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from infer_offline import SpeakerTimeline
from test_bank_models_host import bank_model


def glide_ref(rows, W, clock, bp_n, bp_t, bp_w, spk_w, Fr, n_in, block, hop):
    """The numpy statement of `ddsp_bank_glide` (include/ddsp_amd.h) -> (w_frames (W, Fr, K) fp32, the clocks after the call
    (S,) int64).  rows: W slot numbers, or None for row r = slot r.  clock (S,) int64, bp_n (S,), bp_t (S, P_max) int64, bp_w
    (S, P_max, K) fp32, spk_w (S, K) fp32.  A row whose slot is outside [0, S) is a padding row: weights (1, 0, ..., 0), no clock
    touched.  For a real row c = clock[s] + block, frame t has time tau = float64(c - n_in) + t * hop; without breakpoints every
    frame gets spk_w[s]; with them the first one's weights before it, the last one's from it on, and between two
    w0 + (w1 - w0) * ((tau - t0) / (t1 - t0)) in fp64, rounded to fp32.  Then clock[s] = c."""
    clock = np.array(clock, dtype=np.int64)
    bp_n, bp_t = np.asarray(bp_n, dtype=np.int64), np.asarray(bp_t, dtype=np.int64)
    bp_w, spk_w = np.asarray(bp_w, dtype=np.float32), np.asarray(spk_w, dtype=np.float32)
    S, P_max, K = bp_w.shape
    out = np.zeros((int(W), int(Fr), K), dtype=np.float32)
    for r in range(int(W)):
        s = r if rows is None else int(rows[r])
        if not 0 <= s < S:
            out[r, :, 0] = 1.0
            continue
        c = int(clock[s]) + int(block)
        n = min(max(int(bp_n[s]), 0), P_max)
        for t in range(int(Fr)):
            if n == 0:
                out[r, t] = spk_w[s]
                continue
            tau = np.float64(c - int(n_in)) + np.float64(t) * np.float64(hop)
            p = int(np.searchsorted(bp_t[s, :n].astype(np.float64), tau, side="right"))   # the first breakpoint behind tau
            if p == 0:
                out[r, t] = bp_w[s, 0]
            elif p == n:
                out[r, t] = bp_w[s, n - 1]
            else:
                t0, t1 = np.float64(bp_t[s, p - 1]), np.float64(bp_t[s, p])
                w0, w1 = bp_w[s, p - 1].astype(np.float64), bp_w[s, p].astype(np.float64)
                out[r, t] = (w0 + (w1 - w0) * ((tau - t0) / (t1 - t0))).astype(np.float32)
        clock[s] = c
    return out, clock


def glide_state(S, P_max, K, seed=5):
    """Random slot state: clocks 0, no timelines, random row mixes -> dict of numpy arrays with `ddsp_bank_glide`'s names."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return {"clock": np.zeros(S, dtype=np.int64), "bp_n": np.zeros(S, dtype=np.int32), "bp_t": np.zeros((S, P_max), dtype=np.int64),
            "bp_w": np.zeros((S, P_max, K), dtype=np.float32), "spk_w": rng.uniform(-0.5, 1.5, (S, K)).astype(np.float32)}


def set_points(z, s, times, seed):
    """Slot s of a `glide_state` gets breakpoints at `times` (device samples) with random weights -> those weights (P, K)."""
    w = np.random.Generator(np.random.PCG64(seed)).uniform(-0.5, 1.5, (len(times), z["bp_w"].shape[2])).astype(np.float32)
    z["bp_n"][s] = len(times)
    z["bp_t"][s, :len(times)] = times
    z["bp_w"][s, :len(times)] = w
    return w


# ---- the statement ----------------------------------------------------------------------------------------------------------
def test_statement_is_exact_at_breakpoints_and_holds_outside_them():
    Fr, hop, n_in, block = 37, 512, 36 * 512, 4096
    z = glide_state(2, 4, 3)
    z["clock"][0] = 20000
    first = 20000 + block - n_in                                  # tau of frame 0: 5664
    times = [first - 700, first + 5 * hop, first + 20 * hop, first + 30 * hop + 100]
    w = set_points(z, 0, times, 11)
    got, clock = glide_ref([0], 1, **z, Fr=Fr, n_in=n_in, block=block, hop=hop)
    assert got.dtype == np.float32 and got.shape == (1, Fr, 3)
    assert np.array_equal(got[0, 5], w[1]) and np.array_equal(got[0, 20], w[2])      # tau hits bp_t: the breakpoint's fp32 value
    assert np.array_equal(got[0, 31:], np.broadcast_to(w[3], (6, 3)))                # behind the last one
    want = w[1].astype(np.float64) + (w[2].astype(np.float64) - w[1]) * (hop * 7 / (hop * 15))
    assert np.array_equal(got[0, 12], want.astype(np.float32))
    assert (np.abs(np.diff(got[0, :31, 0])) > 0).all()                                # the ramps move from frame to frame
    # before the first breakpoint: a timeline that starts in the future is held at its first weights
    z["bp_t"][0, :4] += 17 * hop                                  # the first one now lies between frames 15 and 16
    got, _ = glide_ref([0], 1, **z, Fr=Fr, n_in=n_in, block=block, hop=hop)
    assert np.array_equal(got[0, :16], np.broadcast_to(w[0], (16, 3))) and not np.array_equal(got[0, 16], w[0])
    # frames older than time 0 of a fresh timeline (tau < 0) hold the first weights too
    z["clock"][0], z["bp_t"][0, :4] = 0, [0, 3000, 6000, 9000]
    got, clock = glide_ref(None, 2, **z, Fr=Fr, n_in=n_in, block=block, hop=hop)
    assert clock.tolist() == [block, block]
    assert np.array_equal(got[0, :29], np.broadcast_to(w[0], (29, 3)))               # frame 28: tau = 4096 - 18432 + 14336 = 0
    assert not np.array_equal(got[0, 29], w[0])
    # a fractional hop: one breakpoint is a constant mix, and bp_n is clamped to P_max
    z["bp_n"][0] = 9
    a, _ = glide_ref([0], 1, **z, Fr=Fr, n_in=n_in, block=block, hop=512 * 48000 / 44100)
    z["bp_n"][0] = 4
    b, _ = glide_ref([0], 1, **z, Fr=Fr, n_in=n_in, block=block, hop=512 * 48000 / 44100)
    assert np.array_equal(a, b)
    z["bp_n"][0] = 1
    got, _ = glide_ref([0], 1, **z, Fr=Fr, n_in=n_in, block=block, hop=512 * 48000 / 44100)
    assert np.array_equal(got[0], np.broadcast_to(w[0], (Fr, 3)))


def test_statement_without_a_timeline_padding_rows_and_clocks():
    z = glide_state(4, 4, 3)
    z["clock"][:] = [7, 100, 2 ** 40, -5]
    set_points(z, 3, [50], 2)
    before = z["clock"].copy()
    got, clock = glide_ref([2, -1, 0, 4, 3], 5, **z, Fr=6, n_in=4000, block=1000, hop=557.28)
    assert np.array_equal(z["clock"], before)                                        # (the statement copies its clocks)
    for r, s in ((0, 2), (2, 0)):                                                     # bp_n = 0: spk_w over the frames
        assert np.array_equal(got[r], np.broadcast_to(z["spk_w"][s], (6, 3)))
    pad = np.broadcast_to(np.array([1, 0, 0], dtype=np.float32), (6, 3))
    assert np.array_equal(got[1], pad) and np.array_equal(got[3], pad)                # -1 and 4 >= S
    assert np.array_equal(got[4], np.broadcast_to(z["bp_w"][3, 0], (6, 3)))
    assert clock.tolist() == [7 + 1000, 100, 2 ** 40 + 1000, -5 + 1000]               # named slots only; slot 1 untouched
    got2, clock2 = glide_ref(None, 4, **z, Fr=6, n_in=4000, block=1000, hop=557.28)
    assert clock2.tolist() == (before + 1000).tolist() and np.array_equal(got2[3], got[4]) and np.array_equal(got2[0], got[2])


# ---- symbol and ABI ---------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_bound_and_exported(lib_path):
    import hipddsp
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddsp_amd.h")).read(), flags=re.S)
    declared = re.findall(r"\b(ddsp_\w+)\s*\(", text)
    assert declared.count("ddsp_bank_glide") == 1 and "ddsp_bank_glide" in hipddsp.SIGNATURES
    assert hasattr(ctypes.CDLL(lib_path), "ddsp_bank_glide")
    proto = re.search(r"int ddsp_bank_glide\((.*?)\);", text, flags=re.S).group(1)
    assert len(proto.split(",")) == len(hipddsp.SIGNATURES["ddsp_bank_glide"][1]) == 17
    assert "double hop" in proto and hipddsp.SIGNATURES["ddsp_bank_glide"][1][15] is ctypes.c_double
    assert hasattr(hipddsp.Context, "bank_glide_")
    assert hipddsp.ABI_VERSION == 8 and ctypes.CDLL(lib_path).ddsp_abi_version() == 8


# ---- refusals ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(lib_path):
    return bank_model("CombSub", 4, 43)


def _bank(model, n=3, **kw):
    """A bank on the CPU: its state is plain tensors, and no call that passes the refusals could run."""
    import realtime
    return realtime.StreamBank(model, n, 44100, 0.1, 0.04, "cpu", buffer_num=4, use_graph=False, max_mix=3, **kw)


def test_constructor_refusals_and_state(model):
    plain = _bank(model)
    assert plain.glide_breakpoints is None and plain.glide_clock is None and plain.glide_n is None and plain.glide_t is None
    assert plain.glide_w is None and plain._full.w_frames is None and plain.last_mix_w is None
    assert plain._full.mix[1] is plain.spk_w
    for bad in (0, 65, -1, True, 4.0, "4", (4,)):
        with pytest.raises(ValueError, match="glide_breakpoints"):
            _bank(model, glide_breakpoints=bad)
            pytest.fail(f"{bad!r} was accepted")
    with pytest.raises(ValueError, match="glide_breakpoints"):
        _bank(None, models=[model], glide_breakpoints=4)
    for P in (1, 64):
        assert _bank(model, glide_breakpoints=P).glide_t.shape == (3, P)
    bank = _bank(model, glide_breakpoints=4, active_widths=(1, 2))
    assert (bank.glide_clock.dtype, bank.glide_n.dtype, bank.glide_t.dtype, bank.glide_w.dtype) == \
        (torch.int64, torch.int32, torch.int64, torch.float32)
    assert bank.glide_clock.shape == (3,) and bank.glide_n.shape == (3,) and bank.glide_w.shape == (3, 4, 3)
    assert not bank.glide_clock.any() and not bank.glide_n.any()
    for W, rows in [(3, bank._full)] + sorted(bank._compact.items()):
        assert rows.w_frames.shape == (W, bank.frames, 3) and rows.mix[0] is rows.spk_ids and rows.mix[1] is rows.w_frames
    assert sorted(bank._compact) == [1, 2, 3] and bank.graph_builds == 0


def test_set_timeline_writes_the_slots_rows_and_refuses(model):
    bank = _bank(model, glide_breakpoints=4)
    tl = SpeakerTimeline([(0.0, 2), (0.25, {4: 0.5, 2: 0.5}), (0.5, 4)])
    with pytest.raises(ValueError, match="without glide_breakpoints"):
        _bank(model).set_timeline(0, tl)
    bank.set_speaker(1, spk_mix_dict={3: 0.25, 1: 0.75})
    bank.set_timeline(1, tl, at=0.1)
    assert bank.spk_ids[1].tolist() == [2, 4, 1] and int(bank.glide_n[1]) == 3 and int(bank.glide_clock[1]) == 4410
    assert bank.glide_t[1].tolist() == [0, int(round(0.25 * 44100)), 22050, 0] == [0, 11025, 22050, 0]
    assert bank.glide_w[1].tolist() == [[1.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]]
    assert bank.spk_ids[0].tolist() == [1, 1, 1] and not bank.glide_n[[0, 2]].any() and not bank.glide_clock[[0, 2]].any()
    state = [t.clone() for t in (bank.spk_ids, bank.glide_clock, bank.glide_n, bank.glide_t, bank.glide_w)]
    bad = [
        (1, SpeakerTimeline([(0.0, 1), (0.1, 2), (0.2, 1), (0.3, 2), (0.4, 1)]), "glide_breakpoints = 4"),    # more than P_max points
        (1, SpeakerTimeline([(0.100000, 1), (0.100004, 2)]), "both land on sample 4410"),
        (1, SpeakerTimeline([(0.0, {1: 0.25, 2: 0.25, 3: 0.25, 4: 0.25})]), "max_mix = 3"),                  # more ids than max_mix
        (1, SpeakerTimeline([(0.0, 1), (0.5, 5)]), r"\[1, 4\]"),                                            # n_spk = 4
        (3, tl, "slot"), (-1, tl, "slot"), (True, tl, "slot"),
        (1, [(0.0, 1)], "SpeakerTimeline"),
    ]
    for slot, timeline, match in bad:
        with pytest.raises(ValueError, match=match):
            bank.set_timeline(slot, timeline)
            pytest.fail(f"{match!r} was accepted")
    for at in (float("nan"), float("inf"), "0", None, True):
        with pytest.raises(ValueError, match="at must be"):
            bank.set_timeline(1, tl, at=at)
    for t, want in zip((bank.spk_ids, bank.glide_clock, bank.glide_n, bank.glide_t, bank.glide_w), state):
        assert torch.equal(t, want)                                                  # a refused call wrote nothing
    # a plain speaker ends the glide and keeps the clock; reset zeroes the clock and keeps the timeline
    bank.set_timeline(2, tl)
    bank.set_speaker(1, spk_id=3)
    assert int(bank.glide_n[1]) == 0 and int(bank.glide_clock[1]) == 4410 and bank.spk_ids[1].tolist() == [3, 1, 1]
    bank.glide_clock[2] = 999
    bank.reset(2)
    assert int(bank.glide_clock[2]) == 0 and int(bank.glide_n[2]) == 3 and bank.glide_t[2].tolist() == [0, 11025, 22050, 0]
    assert int(bank.glide_clock[1]) == 4410
