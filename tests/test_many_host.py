"""Offline conversion of several files at once, host side (no GPU): `stitch_plan_many` against a `stitch_plan` per file, the
piece table's snapping against `main.split`'s arithmetic, the grouping over several files, and the new symbols' place in the
header, the ctypes table and the library."""
import ctypes
import inspect

import pytest

from infer_offline import group_pieces, piece_table, stitch_plan, stitch_plan_many

BLOCK, SR = 512, 44100


def test_stitch_plan_many_equals_the_per_file_plans():
    """Four files: an odd total (the next base is rounded up), a cross-fade inside a file, an empty file in the middle, a
    piece of one sample; the enhancer-style other output rate on a second pass."""
    starts = [[0, 8, 13], [2, 9], [], [0]]
    lengths = [[9 * BLOCK + 1, 3 * BLOCK, 5 * BLOCK + 3], [7 * BLOCK, 2 * BLOCK + 1], [], [1]]
    for sr_o in (SR, 48000):
        spans, p, fade, total = stitch_plan_many(starts, lengths, BLOCK, SR, sr_o)
        assert len(spans) == 4 and len(p) == len(fade) == 6
        at, end = 0, 0
        for k, (s, n) in enumerate(zip(starts, lengths)):
            pk, fk, tk = stitch_plan(s, n, BLOCK, SR, sr_o)
            base, got_total = spans[k]
            assert base % 2 == 0 and end <= base <= end + 1 and got_total == tk, k
            assert [x - base for x in p[at:at + len(pk)]] == pk and fade[at:at + len(pk)] == fk, k
            if pk:
                assert fade[at] == 0, k                      # nothing fades across files
            at, end = at + len(pk), base + tk
        assert total == end and at == 6
        assert spans[2][1] == 0 and spans[2][0] == spans[3][0]   # the empty file takes no room
        assert fade[1] > 0                                       # (the plan does hold a cross-fade inside file 0)
        assert spans[1][0] == spans[0][1] + (spans[0][1] & 1)
        if sr_o == SR:
            assert spans[0][1] % 2 == 1                          # file 0's total is odd: a gap of one sample in front of file 1
        assert all(a <= b for a, b in zip(p, p[1:]))             # one table for one ddsp_stitch launch


def test_a_file_is_a_list_of_one_file():
    """`file_of_features` is the inverse of `file_features` (CPU tensors: nothing is launched), and the plan of a list of one
    file is the file's own plan at span (0, total)."""
    import torch

    from infer_offline import file_features, file_of_features
    g = torch.Generator().manual_seed(3)
    starts, lens = [0, 8, 13, 19], [9, 3, 5, 7]
    segments = [(s, torch.randn(1, n, 6, generator=g)) for s, n in zip(starts, lens)]
    f0, volume = 100.0 + 300.0 * torch.rand(1, 40, 1, generator=g), torch.rand(1, 40, generator=g)
    files = file_of_features(segments, f0, volume)
    assert files["n_frames"] == [40] and files["pieces"] == [(0, s, n, 0, 0) for s, n in zip(starts, lens)]
    assert files["f0"].shape == files["volume"].shape == (1, 40) and files["f0"].is_contiguous() and files["volume"].is_contiguous()
    assert files["key_factor"].tolist() == [1.0] and files["n_frames_dev"].tolist() == [40] and files["n_frames_dev"].dtype == torch.int32
    got_segments, got_f0, got_volume = file_features(files, 0)
    assert [s for s, _ in got_segments] == starts and all(u is v for (_, u), (_, v) in zip(got_segments, segments))
    assert torch.equal(got_f0, f0) and torch.equal(got_volume, volume) and got_f0.shape == f0.shape
    lengths = [9 * BLOCK + 1, 3 * BLOCK, 5 * BLOCK + 3, 7 * BLOCK]
    for sr_o in (SR, 48000):
        p, fade, total = stitch_plan(starts, lengths, BLOCK, SR, sr_o)
        assert stitch_plan_many([starts], [lengths], BLOCK, SR, sr_o) == ([(0, total)], p, fade, total) and fade[1] > 0


def test_stitch_plan_many_of_nothing():
    assert stitch_plan_many([], [], BLOCK, SR, SR) == ([], [], [], 0)
    assert stitch_plan_many([[], []], [[], []], BLOCK, SR, SR) == ([(0, 0), (0, 0)], [], [], 0)


@pytest.mark.parametrize("starts,lengths,what", [
    ([[0], [0, 5]], [[BLOCK], [BLOCK, 0]], "no samples"),
    ([[0], [5, 0]], [[BLOCK], [BLOCK, BLOCK]], "must ascend"),
    ([[0], [0, 1]], [[BLOCK], [3 * BLOCK, BLOCK]], "cross-fade"),
    ([[0], [0, 1]], [[BLOCK], [BLOCK]], "start frames for"),
])
def test_stitch_plan_many_names_the_file(starts, lengths, what):
    with pytest.raises(ValueError, match=f"file 1: stitch_plan: .*{what}"):
        stitch_plan_many(starts, lengths, BLOCK, SR, SR)
    with pytest.raises(ValueError, match="stitch_plan_many"):
        stitch_plan_many([[0]], [[BLOCK], []], BLOCK, SR, SR)


@pytest.mark.parametrize("sample_rate", [44100, 48000])
def test_piece_table_snaps_as_main_split(sample_rate):
    """An integral hop (512) and a fractional one (48 kHz audio for a 44.1 kHz model: 557.27...): every row against the
    expressions of `main.split` / `_analyse`, written out here."""
    hop_size = BLOCK * sample_rate / SR
    assert float(hop_size).is_integer() == (sample_rate == SR)
    slices = [[(0, 40000), (45000, 90000), (88000, 132300)], [], [(1030, 1100), (557, 1115), (5, 70001)]]
    rows = piece_table(slices, hop_size)
    want = []
    for k, per_file in enumerate(slices):
        for start, end in per_file:
            start_frame, end_frame = int(start // hop_size), int(end // hop_size)
            if end_frame == start_frame:
                continue
            start_sample = int(start_frame * hop_size)
            n_samples = int(end_frame * hop_size) - start_sample
            want.append((k, start_frame, int(n_samples // hop_size) + 1, start_sample, n_samples))
    assert rows == want
    assert [r[0] for r in rows] == [0, 0, 0, 2, 2]                 # (1030, 1100) lies inside one frame: dropped
    for k, start_frame, n_frames, start_sample, n_samples in rows:
        assert start_sample == int(start_frame * hop_size) and n_samples >= 1 and n_frames >= 1
    if sample_rate == 48000:
        assert any(r[3] != r[1] * int(hop_size) for r in rows)     # the fraction does move a start


def test_grouping_over_several_files_takes_every_slice_once():
    slices = [[(0, 9 * BLOCK)], [(0, 20 * BLOCK), (25 * BLOCK, 36 * BLOCK)], [(BLOCK, 3 * BLOCK)], [(0, 5 * BLOCK)] * 3]
    pieces = piece_table(slices, float(BLOCK))
    assert len(pieces) == 7
    for budget, by_samples in ((0, False), (24, False), (1000, False), (12 * BLOCK, True)):
        groups = group_pieces(pieces, budget, by_samples=by_samples)
        assert sorted(i for g in groups for i in g) == list(range(len(pieces)))
        col = 4 if by_samples else 2
        for g in groups:
            assert len(g) == 1 or len(g) * max(pieces[i][col] for i in g) <= budget
    assert all(len(g) == 1 for g in group_pieces(pieces, 0))
    mixed = [{pieces[i][0] for i in g} for g in group_pieces(pieces, 24)]
    assert any(len(m) > 1 for m in mixed)                          # a group holds rows of two files


def test_new_symbols_are_declared_bound_and_exported(lib_path):
    import hipddsp
    lib = ctypes.CDLL(lib_path)
    for name, n_args in (("ddsp_pieces_gather", 18), ("ddsp_volume_gate_files", 14)):
        assert hasattr(lib, name) and len(hipddsp.SIGNATURES[name][1]) == n_args
    gate = inspect.getsource(hipddsp.Context.volume_gate_rows_)
    assert gate.count("self.call(") == 1 and "ddsp_volume_gate_files" in gate and "ddsp_volume_gate_rows" in gate
    params = list(inspect.signature(hipddsp.Context.volume_gate_rows_).parameters)
    assert params[:7] == ["self", "signal", "volume", "start_dev", "n_dev", "threshold_db", "hop"]


def test_public_calls_keep_their_parameter_lists():
    import infer_offline
    want = ["model", "args", "files", "spk_ids", "spk_mix_rows", "threshold_db", "enhancer", "enhancer_adaptive_key", "noise_seed",
            "batch_frames", "noise", "enhancer_batch_samples"]
    assert list(inspect.signature(infer_offline.render_many_device).parameters) == want
    assert list(inspect.signature(infer_offline.analyse_many).parameters) == [
        "args", "audios", "sample_rate", "slices", "units_encoder", "f0_extractor", "keys", "units_batch_samples"]
    assert list(inspect.signature(infer_offline.convert_many_device).parameters)[:7] == [
        "model", "args", "audios", "sample_rate", "units_encoder", "f0_extractor", "spk_ids"]


def test_analyse_many_refuses_a_fractional_hop_before_anything_runs():
    import infer_offline
    from ddsp.vocoder import DotDict
    args = DotDict({"data": {"block_size": BLOCK, "sampling_rate": SR}})
    with pytest.raises(ValueError, match="integral hop"):
        infer_offline.analyse_many(args, [], 48000, None, None, None, 0, None)
