"""The stitch of an offline conversion on the host: `infer_offline.stitch_plan` and the fold rule `ddsp_stitch` implements
(include/ddsp_amd.h) against the reference's `cross_fade` loop recorded in tests/golden/stitch_ref.npz, the plan's errors, and
the command line's options."""
import os

import numpy as np
import pytest

import stitch_cases as SC
from conftest import GOLDEN


def fold(p, fade, pieces, total):
    """The rule of `ddsp_stitch` in numpy: every output sample is a fold over the pieces in order from 0; inside a piece's
    first `fade` samples v = (1 - k) * v + k * x with k = j * (1 / (fade - 1)), the last k exactly 1 and k = 0 for a fade of
    one sample; behind them v = x.  fp64 throughout, one rounding per operation.  This is what the kernel is held to."""
    out = np.zeros(total, dtype=np.float64)
    for at, f, x in zip(p, fade, pieces):
        x = np.asarray(x, dtype=np.float32).astype(np.float64)
        if f == 1:
            k = np.zeros(1)
        else:
            k = np.arange(f, dtype=np.float64) * (1.0 / (f - 1)) if f else np.zeros(0)
            k[-1:] = 1.0
        out[at:at + f] = (1.0 - k) * out[at:at + f] + k * x[:f]
        out[at + f:at + len(x)] = x[f:]
    return out


def load_case(z, name):
    """-> (sr, sr_o, starts, pieces [fp32 arrays], result fp64) of one case of the fixture."""
    sr, sr_o = (int(v) for v in z[f"{name}_rates"])
    lengths = [int(n) for n in z[f"{name}_lengths"]]
    flat = z[f"{name}_pieces"]
    ends = np.cumsum([0] + lengths)
    return sr, sr_o, [int(s) for s in z[f"{name}_starts"]], [flat[a:b] for a, b in zip(ends[:-1], ends[1:])], z[f"{name}_result"]


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "stitch_ref.npz"))


def test_fixture_holds_the_listed_cases(ref):
    assert list(ref["names"]) == list(SC.CASES) and int(ref["block"]) == SC.BLOCK
    for name, (rates, rows) in SC.CASES.items():
        sr, sr_o, starts, pieces, result = load_case(ref, name)
        assert (sr, sr_o) == rates and list(zip(starts, (len(x) for x in pieces))) == rows
        assert all(x.dtype == np.float32 and 1 <= len(x) <= 40 for x in pieces) and result.dtype == np.float64
        for x, y in zip(pieces, SC.pieces(name)):
            assert np.array_equal(x, y)
    kinds = {f for _, f, _ in SC.EXPECTED.values() for f in f}
    assert {0, 1} <= kinds and max(kinds) >= 2   # abutting, a one-sample fade, a longer one


@pytest.mark.parametrize("name", list(SC.CASES))
def test_stitch_plan_and_fold_equal_the_reference_loop(ref, name):
    import infer_offline
    sr, sr_o, starts, pieces, result = load_case(ref, name)
    p, fade, total = infer_offline.stitch_plan(starts, [len(x) for x in pieces], SC.BLOCK, sr, sr_o)
    assert (list(p), list(fade), total) == SC.EXPECTED[name]
    got = fold(p, fade, pieces, total)
    assert got.shape == result.shape and np.array_equal(got, result)


def test_a_one_sample_fade_keeps_the_earlier_sample(ref):
    _, _, _, pieces, result = load_case(ref, "fades")
    p, fade, _ = SC.EXPECTED["fades"]
    assert fade[2] == 1 and result[p[2]] == np.float64(pieces[1][p[2] - p[1]]) and result[p[2] + 1] == np.float64(pieces[2][1])


def test_gaps_and_leading_silence_are_zero(ref):
    result = load_case(ref, "lead_gap_abut")[4]
    assert not result[:8].any() and not result[16:20].any() and result[8:16].all()


@pytest.mark.parametrize("starts,lengths,word", [
    ([0, 2], [30, 3], "cross-fade"),      # 22 samples of overlap, 3 samples long: len < fade
    ([0, 5], [8, 0], "no samples"),       # len == 0
    ([0, 6, 5], [8, 8, 8], "ascend"),     # descending p
])
def test_stitch_plan_refuses(starts, lengths, word):
    import infer_offline
    with pytest.raises(ValueError, match=word) as e:
        infer_offline.stitch_plan(starts, lengths, SC.BLOCK, 44100, 44100)
    assert f"piece {len(starts) - 1}" in str(e.value)


def test_stitch_checks_the_pieces_against_the_plan_before_any_device_call():
    """`stitch` on host tensors of the wrong length raises ValueError from its own check: no context, no launch."""
    import torch

    import infer_offline
    plan = infer_offline.stitch_plan([0, 2], [8, 8], SC.BLOCK, 44100, 44100)
    with pytest.raises(ValueError, match="the plan at 16"):
        infer_offline.stitch([torch.zeros(8), torch.zeros(7)], plan)
    with pytest.raises(ValueError, match="piece 1"):
        infer_offline.stitch([torch.zeros(9), torch.zeros(7)], plan)      # piece 1 would now fade over one sample
    with pytest.raises(ValueError, match="1 pieces"):
        infer_offline.stitch([torch.zeros(8)], plan)


def test_main_parse_args_takes_the_reference_options_and_defaults():
    import main
    cmd = main.parse_args(["-m", "model.pt", "-i", "in.wav", "-o", "out.wav"])
    assert vars(cmd) == {"model_path": "model.pt", "input": "in.wav", "output": "out.wav", "spk_id": 1, "spk_mix_dict": "None",
                         "key": 0, "enhance": "true", "pitch_extractor": "crepe", "f0_min": 50, "f0_max": 1100, "threhold": -60,
                         "enhancer_adaptive_key": 0, "sampling_rate": 44100}
    cmd = main.parse_args(["-m", "a", "-i", "b", "-o", "c", "-id", "3", "-mix", "{1: 0.5, 2: 0.5}", "-k", "-5", "-e", "false",
                           "-pe", "ac", "-fmin", "65", "-fmax", "800", "-th", "-45", "-eak", "2", "-sr", "48000"])
    assert (cmd.spk_id, cmd.spk_mix_dict, cmd.key, cmd.enhance, cmd.pitch_extractor, cmd.f0_min, cmd.f0_max, cmd.threhold,
            cmd.enhancer_adaptive_key, cmd.sampling_rate) == ("3", "{1: 0.5, 2: 0.5}", "-5", "false", "ac", "65", "800", "-45",
                                                              "2", 48000)
    for missing in (["-i", "b", "-o", "c"], ["-m", "a", "-o", "c"], ["-m", "a", "-i", "b"]):
        with pytest.raises(SystemExit):
            main.parse_args(missing)


def test_pcm16_rounds_and_clips():
    import main
    got = main.pcm16(np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, 1.5 / 32768, 2.5 / 32768, -3.0]))
    assert got.dtype == np.int16 and got.tolist() == [0, 16384, -16384, 32767, -32768, 32767, 2, 2, -32768]
