"""The validation case shared by tests/golden/make_golden_solver.py and the trainer tests: five utterances of three speakers,
as plain numpy (no GPU, no library).  The fixture tests/golden/ref_solver.npz holds what the reference's `solver.test` made of
them."""
import os

import numpy as np

SR, HOP, N_UNIT = 44100, 512, 256
N_SPK = 3
FRAMES = [5, 9, 17, 33, 40]                 # every utterance holds fft_max = 2048 samples (5 * 512 = 2560)
SPK = [1, 2, 3, 3, 1]                       # 3 -> (3 + 1) % 3 = 1: the wrap; 2 -> 0 -> 1: the zero rule
NAMES = ["1/a", "2/b", "3/c", "3/d", "1/e"]
F0_STATS = {"1": 5.2, "2": 5.6, "3": 4.9}   # mean log f0 per speaker (about 181, 270 and 134 Hz)
SCALES = [256, 777, 1531, 2047]             # the smallest and the largest scale the loss can draw, and two between
FFT_MIN, FFT_MAX, N_SCALE = 256, 2048, 4
UNVOICED = {0: [0, 1], 2: [3, 4, 5, 16], 4: [39]}      # utterance -> frames with f0 == 0
TAIL = 64                                   # samples after the last frame: the file's duration then floors to FRAMES[i] frames
INPUT_SEED = 8100


def make_utterances():
    """[{name, spk_id, units (n, 256), f0 (n,), volume (n,), audio (n * HOP + TAIL,), noise (n * HOP,)}] float32, seeded."""
    import synthetic
    out = []
    for i, n in enumerate(FRAMES):
        inp = synthetic.make_inputs(INPUT_SEED + i, 1, n)
        f0 = inp["f0"][0, :, 0].numpy().copy()
        f0[UNVOICED.get(i, [])] = 0.0
        rng = np.random.Generator(np.random.PCG64(INPUT_SEED + 100 + i))
        t = np.arange(n * HOP + TAIL) / SR
        audio = (0.05 * rng.standard_normal(n * HOP + TAIL) + 0.2 * np.sin(2 * np.pi * (150.0 + 40 * i) * t)).astype(np.float32)
        out.append({"name": NAMES[i], "spk_id": SPK[i], "units": inp["units"][0].numpy(), "f0": f0,
                    "volume": inp["volume"][0].numpy(), "audio": audio, "noise": inp["noise"][0].numpy()})
    return out


def records(z):
    """The fixture's utterances as `AudioDataset(records=...)` takes them."""
    return [{"name": str(name), "audio": z[f"audio_{i}"], "duration": len(z[f"audio_{i}"]) / SR, "spk_id": int(z["spk"][i]),
             "f0": z[f"f0_{i}"], "volume": z[f"volume_{i}"], "units": [z[f"units_{i}"]]} for i, name in enumerate(z["names"])]


def f0_stats(z):
    return {str(k): float(v) for k, v in zip(z["f0_stats_keys"], z["f0_stats_values"])}


def vc_f0_numpy(f0, lfo_src, lfo_tgt):
    """exp(lfo_tgt * ln(f0) / lfo_src) in float32 with 0 staying 0: the numpy restatement of `solver.py:54`."""
    f0 = np.asarray(f0, dtype=np.float32)
    out = np.zeros_like(f0)
    v = f0 > 0
    out[v] = np.exp(np.float32(lfo_tgt) * np.log(f0[v]) / np.float32(lfo_src))
    return out


def load():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_solver.npz"))
