"""Shapes and seeds of tests/golden/ref_volume_frac.npz (the same tables as tests/golden/make_golden_rates.py): volume
extraction and unit alignment at the hop `block_size * sample_rate / model_rate` of an input at another rate than the
model's (main.py:72,109; gui.py:94)."""
import numpy as np
import torch

# 512-sample model hop at 44.1 kHz seen from 48 / 22.05 / 16 kHz inputs, a 48 kHz model seen from 32 kHz, a plain 441
VOLUME_HOPS = [512 * 48000 / 44100, 512 * 22050 / 44100, 512 * 16000 / 44100, 512 * 32000 / 48000, 441.0]


def volume_lengths(h):
    """Signal lengths for hop h: a second at 48 kHz, an odd length, one just past a frame boundary (the last block holds
    one real sample and the reflected tail), one just below a frame boundary, and the shortest the reflect pad allows."""
    return [48000, 12345, int(20 * h) + 1, int(7 * h) - 1, int((h + 1) // 2) + 1]


def volume_audio(i, j):
    h = VOLUME_HOPS[i]
    T = volume_lengths(h)[j]
    return np.random.Generator(np.random.PCG64(1300 + 10 * i + j)).uniform(-1, 1, size=T).astype(np.float32), h


# alignment tail of Units_Encoder.encode at the 48 kHz hop: (n_samples, Lu, C); 55 700 = 100 * 557 gives 100 frames at the
# fractional hop and 101 at its truncation
ALIGN_SR = 48000
ALIGN_HOP = 512 * 48000 / 44100
ALIGN_CASES = [(55700, 120, 8), (48000, 101, 16), (96000, 30, 4)]


def align_input(i):
    n, Lu, C = ALIGN_CASES[i]
    units = np.random.Generator(np.random.PCG64(1400 + i)).standard_normal((1, Lu, C)).astype(np.float32)
    return torch.from_numpy(units), n


def volume_reference(audio, hop_size):
    """The reference's volume formula (ddsp/vocoder.py:124-137) restated for the CPU chains of the tests, Python floats
    throughout; held to ref_volume_frac.npz by tests/test_rates_host.py."""
    n_frames = int(len(audio) // hop_size) + 1
    audio = np.pad(audio, (int(hop_size // 2), int((hop_size + 1) // 2)), mode="reflect")
    audio2 = audio ** 2
    return np.sqrt(np.array([np.mean(audio2[int(n * hop_size): int((n + 1) * hop_size)]) for n in range(n_frames)]))
