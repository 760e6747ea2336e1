"""Generates tests/golden/slicer_ref.npz by running the REFERENCE's `slicer.Slicer` in this container.

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_slicer.py
The reference's `slicer.py` imports librosa and torchaudio, which the image lacks.  Stand-ins of our own replace them:
`torchaudio` is empty (only `chunks2audio` uses it), `librosa.to_mono` is the channel mean and `librosa.feature.rms` is the
fp32 numpy restatement of tests/slicer_cases.py in the pad mode of the run ('constant': librosa >= 0.10, 'reflect': before).
So the tagging state machine and the chunk assembly are the reference's own code run on its own class; the RMS is pinned
against its documented definition.
Every case of tests/slicer_cases.py runs under both pad modes.  Recorded per case and mode: the signal's length and the sum
of its squares (the signal itself is seeded: `slicer_cases.signal`), the constructor's rounded values as the reference object
holds them, the chunks of the returned dict as (K, 3) rows, and the line numbers of `Slicer.slice` that ran (a line trace).
The maker asserts from those lines that the cases between them took every branch of the state machine and of the chunk
assembly, and that the condition on the cases holds (`slicer_cases.check_conditions`).
The reference tree never travels to the GPU box; only the .npz and this script are committed."""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

from make_golden import REF, save  # noqa: E402
import slicer_cases as SC  # noqa: E402

MODE = ["constant"]

# lines of the reference's slicer.py whose execution shows a branch: the early return, the cleared run, the three
# placement branches each from frame 0 and from a later frame, the trailing tag, no tags, the leading voiced chunk, the
# closing chunk
BRANCH_LINES = {"early": 33, "cleared": 52, "le_keep_zero": 58, "le_keep": 60, "le_2keep_zero": 68, "le_2keep": 71,
                "longer_zero": 77, "longer": 79, "trailing": 87, "no_tags": 90, "lead_voiced_chunk": 95, "closing_chunk": 107}


def _stand_ins():
    lib = types.ModuleType("librosa")
    lib.to_mono = lambda y: np.mean(y, axis=0)
    lib.feature = types.ModuleType("librosa.feature")
    lib.feature.rms = lambda y, frame_length, hop_length: SC.rms(y, frame_length, hop_length, MODE[0], np.float32)[None]
    sys.modules["librosa"] = lib
    sys.modules["librosa.feature"] = lib.feature
    sys.modules["torchaudio"] = types.ModuleType("torchaudio")


def _traced(fn, *args):
    """fn(*args) -> (result, the set of line numbers of fn's own code that ran)."""
    code, lines = fn.__code__, set()

    def tracer(frame, event, arg):
        if frame.f_code is not code:
            return None
        if event == "line":
            lines.add(frame.f_lineno)
        return tracer

    sys.settrace(tracer)
    try:
        out = fn(*args)
    finally:
        sys.settrace(None)
    return out, lines


def main():
    _stand_ins()
    sys.path.insert(0, REF)
    import slicer as RS   # the reference module
    sys.path.remove(REF)
    assert RS.__file__.startswith(REF)

    g = {"names": np.array(list(SC.CASES)), "pad_modes": np.array(SC.PAD_MODES)}
    seen = set()
    for name, (pset, plan, extra, seed, zeros) in SC.CASES.items():
        x = SC.signal(name)
        obj = RS.Slicer(**SC.PARAMS[pset])
        fr = SC.frames_of(SC.PARAMS[pset])
        assert (obj.hop_size, obj.win_size, obj.min_length, obj.min_interval, obj.max_sil_kept, obj.threshold) == \
            (fr["hop"], fr["win"], fr["min_length"], fr["min_interval"], fr["max_sil_kept"], fr["threshold"])
        g[f"{name}_frames"] = np.array([obj.hop_size, obj.win_size, obj.min_length, obj.min_interval, obj.max_sil_kept])
        g[f"{name}_threshold"] = np.float64(obj.threshold)
        g[f"{name}_n"] = x.shape[0]
        g[f"{name}_energy"] = np.float64(np.sum(x.astype(np.float64) ** 2))
        for mode in SC.PAD_MODES:
            MODE[0] = mode
            SC.check_conditions(name, mode)
            out, lines = _traced(obj.slice, x)
            taken = {k for k, ln in BRANCH_LINES.items() if ln in lines}
            seen |= taken
            g[f"{name}_{mode}_chunks"] = SC.chunks_of_dict(out)
            g[f"{name}_{mode}_lines"] = np.array(sorted(lines))
            print(f"{name:9s} {mode:8s} n {x.shape[0]:6d} chunks {len(out):2d} {sorted(taken)}")
    missing = set(BRANCH_LINES) - seen
    assert not missing, f"no case took {sorted(missing)}"
    save("slicer_ref.npz", **g)


if __name__ == "__main__":
    main()
