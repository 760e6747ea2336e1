"""The cases of tests/golden/stitch_ref.npz (made by tests/golden/make_golden_stitch.py, read by tests/test_stitch_host.py and
tests/test_gpu_stitch.py): per case the rates (sr, sr_o) and the pieces as (start_frame, samples), block = 4.

With sr_o == sr a piece starts at output sample 4 * start_frame; at 48000 / 44100 at round(start_frame * 4 * 48000 / 44100),
which lands on odd samples too.  What each case is there for:
  lead_gap_abut   leading silence (8 samples), a gap (4), two abutting pieces (fade 0), the last of one sample
  fades           a fade of 10; a fade of exactly 1 (keeps the earlier sample); a one-sample piece that is all fade
  double_overlap  the third piece overlaps the two before it ((0, 30), (24, 10), (28, 20))
  double_up       the same at 48000 / 44100: (0, 33), (26, 10), (30, 20)
  up_mix          at 48000 / 44100: abutting at an odd sample, a fade of 2, a piece that is all fade (36 of 36)
  single          one piece behind leading silence, at 48000 / 44100
  empty           no piece: a result of length 0
"""
import numpy as np

BLOCK = 4
SAME, UP = (44100, 44100), (44100, 48000)
CASES = {
    "lead_gap_abut": (SAME, [(2, 8), (5, 16), (9, 8), (11, 1)]),
    "fades": (SAME, [(0, 30), (5, 25), (11, 9), (13, 1)]),
    "double_overlap": (SAME, [(0, 30), (6, 10), (7, 20)]),
    "double_up": (UP, [(0, 33), (6, 10), (7, 20)]),
    "up_mix": (UP, [(1, 13), (4, 20), (8, 40), (9, 36)]),
    "single": (UP, [(3, 17)]),
    "empty": (SAME, []),
}
# (p, fade) of every piece and the total, worked out by hand from the rule: the generator and the host test hold
# `stitch_plan` and the reference loop to them
EXPECTED = {
    "lead_gap_abut": ([8, 20, 36, 44], [0, 0, 0, 0], 45),
    "fades": ([0, 20, 44, 52], [0, 10, 1, 1], 53),
    "double_overlap": ([0, 24, 28], [0, 6, 6], 48),
    "double_up": ([0, 26, 30], [0, 7, 6], 50),
    "up_mix": ([4, 17, 35, 39], [0, 0, 2, 36], 75),
    "single": ([13], [0], 30),
    "empty": ([], [], 0),
}


def pieces(name):
    """The case's pieces: seeded fp32 noise of the listed lengths (the fixture stores them; this is how they were drawn)."""
    rng = np.random.Generator(np.random.PCG64(4100 + list(CASES).index(name)))
    return [(0.5 * rng.standard_normal(n)).astype(np.float32) for _, n in CASES[name][1]]
