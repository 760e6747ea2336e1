"""CPU side of the device-rate / enhancer chain of `realtime.StreamRenderer`: the size and key arithmetic it takes from the
reference's `gui.py` / `enhancer.py`, held to those formulas (restated here verbatim) at the sizes of the GUI's defaults,
BASELINE config #5 and a 48 kHz device; and the tests' own CPU volume formula held to the reference's outputs."""
import os

import numpy as np
import pytest
import torch

import rates_cases as RC
from conftest import GOLDEN

MODEL_SR, BLOCK_SIZE = 44100, 512
# (device rate, block_time, crossfade_time, buffer_num): gui.py Config defaults, BASELINE config #5, both at 48 kHz
SHAPES = [(44100, 1.5, 0.03, 2), (44100, 0.2, 0.04, 4), (48000, 1.5, 0.03, 2), (48000, 0.2, 0.04, 4), (22050, 0.5, 0.05, 3)]


def _gui_sizes(samplerate, block_time, crossfade_time, buffer_num):
    """gui.py:317-326 (`set_values`) and gui.py:88-94 (`SvcDDSP.infer`)."""
    block_frame = int(block_time * samplerate)
    crossfade_frame = int(crossfade_time * samplerate)
    sola_search_frame = int(0.01 * samplerate)
    last_delay_frame = int(0.02 * samplerate)
    input_frames = max(block_frame + crossfade_frame + sola_search_frame + 2 * last_delay_frame, (1 + buffer_num) * block_frame)
    f_safe_prefix_pad_length = block_time * buffer_num - crossfade_time - 0.01 - 0.02
    hop_size = BLOCK_SIZE * samplerate / MODEL_SR
    if f_safe_prefix_pad_length > 0.03:
        silence_front = f_safe_prefix_pad_length - 0.03
    else:
        silence_front = 0
    n_frames = int(input_frames // hop_size) + 1          # Volume_Extractor.extract of the window (ddsp/vocoder.py:125)
    start_frame = int(silence_front * MODEL_SR / BLOCK_SIZE)   # enhancer.py:27
    return input_frames, hop_size, n_frames, silence_front, start_frame


@pytest.mark.parametrize("shape", SHAPES)
def test_size_arithmetic_matches_gui(shape):
    import realtime
    sr, bt, xt, bn = shape
    n_in, hop, frames, sf, cut = _gui_sizes(sr, bt, xt, bn)
    assert realtime.input_frames(sr, bt, xt, bn) == n_in
    assert realtime.hop_size(BLOCK_SIZE, sr, MODEL_SR) == hop
    assert realtime.window_frames(n_in, hop) == frames
    assert realtime.silence_front(bt, bn, xt) == sf
    assert realtime.key_cut_frames(sf, MODEL_SR, BLOCK_SIZE) == cut
    if sr == MODEL_SR:
        assert float(hop).is_integer() and frames == n_in // BLOCK_SIZE + 1     # what the renderer computed before
    assert float(hop).is_integer() == (sr in (44100, 22050))                   # 22.05 kHz: 256.0, an integral float


def test_known_sizes():
    import realtime
    # config #5: 44 100-sample window, 87 frames, 0.70 s silent front = 60 frames
    assert realtime.input_frames(44100, 0.2, 0.04, 4) == 44100
    assert realtime.window_frames(44100, realtime.hop_size(512, 44100, 44100)) == 87
    assert realtime.key_cut_frames(realtime.silence_front(0.2, 4, 0.04), 44100, 512) == 60
    # the GUI's defaults at 48 kHz: 216 000-sample window at hop 557.29
    h = realtime.hop_size(512, 48000, 44100)
    assert abs(h - 557.2789) < 1e-4
    assert realtime.input_frames(48000, 1.5, 0.03, 2) == 216000
    assert realtime.window_frames(216000, h) == 216000 * 44100 // (512 * 48000) + 1 == 388
    assert realtime.silence_front(0.1, 1, 0.05) == 0                               # no room for a silent front


def _reference_auto_key(f0):
    """enhancer.py:34-38 on a (1, Fr, 1) torch track."""
    return max(0, np.ceil(12 * np.log2(float(torch.max(f0) / 760))))


@pytest.mark.parametrize("peak,key", [(759.0, 0), (760.0, 0), (761.0, 1), (1100.0, 7), (760.0 * 2 ** (5 / 12), 5),
                                      (1520.0, 12), (1520.5, 13), (100.0, 0)])
def test_auto_key_matches_enhancer_rule(peak, key):
    import realtime
    f0 = torch.full((1, 30, 1), 200.0)
    f0[0, 17, 0] = peak
    assert _reference_auto_key(f0) == key
    assert realtime.auto_key(float(torch.max(f0))) == key
    assert isinstance(realtime.auto_key(peak), int)
    assert realtime.auto_key(0.0) == 0                                             # an unvoiced window


def test_output_rate():
    import realtime

    class _Enh:
        enhancer_sample_rate = 44100
    assert realtime.output_rate(44100) == 44100
    assert realtime.output_rate(32000, None) == 32000
    assert realtime.output_rate(32000, _Enh()) == 44100


def test_cpu_volume_formula_matches_reference():
    """The volume formula the CPU chains of tests/test_gpu_stream_chain.py use, against the reference's own outputs."""
    z = np.load(os.path.join(GOLDEN, "ref_volume_frac.npz"))
    for i, h in enumerate(RC.VOLUME_HOPS):
        for j in range(len(RC.volume_lengths(h))):
            audio, hop = RC.volume_audio(i, j)
            assert np.array_equal(RC.volume_reference(audio, hop), z[f"vol_{i}_{j}"]), (i, j)


def test_golden_frame_counts_are_the_fractional_ones():
    """The fixture's frame counts are int(T // h) + 1 at the fractional hop, which truncating the hop does not give for
    every case (the failure the fractional entry point fixes)."""
    z = np.load(os.path.join(GOLDEN, "ref_volume_frac.npz"))
    differ = 0
    for i, h in enumerate(RC.VOLUME_HOPS):
        for j, T in enumerate(RC.volume_lengths(h)):
            assert z[f"vol_{i}_{j}"].shape == (int(T // h) + 1,)
            differ += int(T // h) != T // int(h)
    assert differ > 0
    n, _, _ = RC.ALIGN_CASES[0]
    assert z["align_0"].shape[1] == int(n // RC.ALIGN_HOP) + 1 != n // int(RC.ALIGN_HOP) + 1
