"""Generates tests/golden/stitch_ref.npz by running the REFERENCE's `cross_fade` (main.py:50-57) in this container.

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stitch.py
The reference's `main.py` imports librosa, soundfile, tqdm, its slicer, its ddsp package and its enhancer at the top; none of
them is needed by `cross_fade`, and several are not installed, so empty stand-in modules carrying the imported names take
their place while the module is loaded (its `__main__` block does not run on import).  The stitch itself lives in that
`__main__` block (main.py:165-173) and cannot be imported: `reference_stitch` below drives the reference's `cross_fade` the
way those lines do - silence and `np.append` for a piece at or behind the end of the result, `cross_fade` at `current_length
+ silent_length` otherwise.
Every case of tests/stitch_cases.py is recorded: the rates, the start frames, the lengths, the pieces (fp32, concatenated)
and the float64 result.  The maker asserts the hand-worked positions, fades and totals of `stitch_cases.EXPECTED`.
The reference tree never travels to the GPU box; only the .npz and this script are committed."""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

from make_golden import REF, save  # noqa: E402
import stitch_cases as SC  # noqa: E402

STAND_INS = {"librosa": (), "soundfile": (), "slicer": ("Slicer",), "ddsp": (), "ddsp.core": ("upsample",), "enhancer": ("Enhancer",),
             "ddsp.vocoder": ("load_model", "F0_Extractor", "Volume_Extractor", "Units_Encoder"), "tqdm": ("tqdm",)}


def reference_main():
    """The reference's main.py as a module, loaded under stand-ins for its imports; sys.modules is put back afterwards."""
    kept = {name: sys.modules.get(name) for name in STAND_INS}
    for name, attrs in STAND_INS.items():
        mod = types.ModuleType(name)
        for a in attrs:
            setattr(mod, a, None)
        sys.modules[name] = mod
    try:
        spec = importlib.util.spec_from_file_location("reference_main", os.path.join(REF, "main.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for name, old in kept.items():
            if old is None:
                del sys.modules[name]
            else:
                sys.modules[name] = old
    return mod


def reference_stitch(cross_fade, starts, pieces, block, sr, sr_o):
    """main.py:165-173 over prepared pieces -> (result, [(position, fade)] per piece)."""
    result, current, placed = np.zeros(0), 0, []
    for start, out in zip(starts, pieces):
        silent = round(start * block * sr_o / sr) - current
        if silent >= 0:
            result = np.append(result, np.zeros(silent))
            result = np.append(result, out)
        else:
            result = cross_fade(result, out, current + silent)
        placed.append((current + silent, max(0, -silent)))
        current = current + silent + len(out)
    assert current == len(result)
    return result, placed


def main():
    ref = reference_main()
    assert ref.__file__.startswith(REF)
    g = {"names": np.array(list(SC.CASES)), "block": SC.BLOCK}
    for name, ((sr, sr_o), rows) in SC.CASES.items():
        xs = SC.pieces(name)
        starts = [s for s, _ in rows]
        assert [len(x) for x in xs] == [n for _, n in rows] and all(1 <= len(x) <= 40 for x in xs)
        result, placed = reference_stitch(ref.cross_fade, starts, xs, SC.BLOCK, sr, sr_o)
        p, fade, total = SC.EXPECTED[name]
        assert placed == list(zip(p, fade)) and len(result) == total and result.dtype == np.float64, (name, placed, len(result))
        g[f"{name}_rates"] = np.array([sr, sr_o])
        g[f"{name}_starts"] = np.array(starts, dtype=np.int64)
        g[f"{name}_lengths"] = np.array([len(x) for x in xs], dtype=np.int64)
        g[f"{name}_pieces"] = np.concatenate(xs) if xs else np.zeros(0, np.float32)
        g[f"{name}_result"] = result
        print(f"{name:15s} pieces {len(xs)} total {total:3d} fades {fade}")
    save("stitch_ref.npz", **g)


if __name__ == "__main__":
    main()
