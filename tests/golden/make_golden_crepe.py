"""Generates tests/golden/ref_crepe_postfilter.npz by running the REFERENCE's own `F0_Extractor('crepe').extract`
(ddsp/vocoder.py) with the placeholders of make_golden.py.  torchcrepe is not installed, so its two names the reference uses
are stand-ins: `torchcrepe.predict` returns a recorded (f0, periodicity) track of 1 + T16 // 80 frames and records the 16 kHz
length T16 it was handed; `torchcrepe.threshold.At` is restated (f0 = NaN where periodicity < value).  The resampler is a
stand-in that records nothing but returns ceil(T * 16000 / sr) samples (torchaudio's output length).  Everything else - the
silence_front crop, MedianPool1d, MaskedAvgPool1d, the re-timing, the start pad and uv_interp - is the reference's code.

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_crepe.py
Stored per case i: f0_in_<i>, pd_in_<i> (the recorded track), out_<i> (the reference's result, fp32), and the arrays
sr, hop (fp64), T, silence_front, uv_interp, f0_min, T16, n_frames, start_frame over the cases."""
import math
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden import REF, _placeholders, save  # noqa: E402

# (sr, hop, T, silence_front, uv_interp, track kind)
CASES = [
    (44100, 512, 44100, 0.0, False, "voiced"),
    (44100, 512, 44100, 0.0, True, "voiced"),
    (48000, 512 * 48000 / 44100, 72000, 0.0, True, "voiced"),
    (48000, 512 * 48000 / 44100, 216000, 1.47, True, "voiced"),          # the GUI window: 4.5 s, silence_front 1.47 s
    (48000, 512 * 48000 / 44100, 216000, 1.47, False, "voiced"),
    (44100, 512, 66150, 0.5, False, "gaps"),
    (44100, 512, 22050, 0.0, True, "unvoiced"),
    (44100, 512, 22050, 0.0, False, "unvoiced"),
    (44100, 512, 441, 0.0, True, "voiced"),                              # the shortest accepted length: 160 samples, 3 frames
    (16000, 160, 16000, 0.0, True, "gaps"),
]
F0_MIN, F0_MAX = 65, 800


def track(kind, fr, seed):
    """A recorded (f0, periodicity) track: NaN runs in f0, periodicity crossing 0.05, runs with no voiced frame."""
    rng = np.random.default_rng(seed)
    t = np.arange(fr)
    f0 = (180 + 80 * np.sin(2 * np.pi * t / 97) + 3 * rng.standard_normal(fr)).astype(np.float32)
    pd = (0.05 + 0.04 * np.sin(2 * np.pi * t / 23 + 0.7) + 0.02 * rng.standard_normal(fr)).astype(np.float32)
    if kind == "voiced":
        pd = np.abs(pd + 0.03).astype(np.float32)
        f0[fr // 3: fr // 3 + 3] = np.nan
    elif kind == "gaps":
        for s in range(5, fr, 40):
            pd[s: s + 9] = 0.01                                          # a window with no voiced frame
        f0[fr // 2: fr // 2 + 4] = np.nan
    else:
        pd = np.minimum(pd, 0.04).astype(np.float32)
    return f0, pd


def main():
    import warnings
    warnings.simplefilter("ignore")
    _placeholders()
    tc = sys.modules["torchcrepe"]
    seen = {}
    current = {}

    def predict(audio, sr, hop, fmin, fmax, pad=True, model="full", batch_size=None, device="cpu", return_periodicity=False):
        assert sr == 16000 and hop == 80 and pad and return_periodicity and (fmin, fmax) == (F0_MIN, F0_MAX)
        T16 = audio.shape[-1]
        seen["T16"] = T16
        f0, pd = track(current["kind"], 1 + T16 // 80, current["seed"])
        current["f0"], current["pd"] = f0, pd
        return torch.from_numpy(f0.copy())[None], torch.from_numpy(pd.copy())[None]

    class At:
        def __init__(self, value):
            self.value = value

        def __call__(self, pitch, periodicity):
            out = pitch.clone()
            out[periodicity < self.value] = float("nan")
            return out

    tc.predict = predict
    tc.threshold = type(sys)("torchcrepe.threshold")
    tc.threshold.At = At

    class Resample16k(torch.nn.Module):
        def __init__(self, sr):
            super().__init__()
            self.sr = sr

        def forward(self, x):
            return torch.zeros(x.shape[0], -(-x.shape[-1] * 16000 // self.sr))

    for k in [k for k in sys.modules if k == "ddsp" or k.startswith("ddsp.") or k.startswith("encoder")]:
        del sys.modules[k]
    sys.path.insert(0, REF)
    import ddsp.vocoder as RV
    sys.path.remove(REF)

    out = {k: [] for k in ("sr", "hop", "T", "silence_front", "uv_interp", "f0_min", "T16", "n_frames", "start_frame")}
    for i, (sr, hop, T, sf, uv, kind) in enumerate(CASES):
        RV.CREPE_RESAMPLE_KERNEL[str(sr)] = Resample16k(sr)
        ex = RV.F0_Extractor("crepe", sr, hop, F0_MIN, F0_MAX)
        current.update(kind=kind, seed=100 + i)
        audio = np.zeros(T, dtype=np.float32)
        f0 = ex.extract(audio, uv_interp=uv, device="cpu", silence_front=sf)
        n_frames = int(T // hop) + 1
        start_frame = int(sf * sr / hop)
        assert f0.dtype == np.float32 and f0.shape == (n_frames,), (f0.dtype, f0.shape)
        out[f"f0_in_{i}"] = current["f0"]
        out[f"pd_in_{i}"] = current["pd"]
        out[f"out_{i}"] = f0
        for k, v in (("sr", sr), ("hop", float(hop)), ("T", T), ("silence_front", sf), ("uv_interp", int(uv)),
                     ("f0_min", F0_MIN), ("T16", seen["T16"]), ("n_frames", n_frames), ("start_frame", start_frame)):
            out[k].append(v)
        print(i, sr, hop, T, sf, uv, kind, "T16", seen["T16"], "frames", len(current["f0"]), "->", f0.shape, flush=True)
    for k in ("sr", "hop", "T", "silence_front", "uv_interp", "f0_min", "T16", "n_frames", "start_frame"):
        out[k] = np.array(out[k], dtype=np.float64 if k in ("hop", "silence_front") else np.int64)
    assert all(math.isfinite(float(np.nansum(out[f"out_{i}"]))) for i in range(len(CASES)))
    save("ref_crepe_postfilter.npz", **out)


if __name__ == "__main__":
    main()
