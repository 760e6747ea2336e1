"""The case of tests/golden/ref_framemix.npz, shared by its maker (tests/golden/make_golden_framemix.py) and the tests: a speaker
mix whose weights change from frame to frame.  B * Fr = 111 rows: no multiple of a GEMM tile, and batch rows straddle tiles."""
import numpy as np

B, FR, N_SPK = 3, 37, 8
IDS = (2, 5, 8)                      # dict order = slot order; 8 is the table's last row
NAMES = ("CombSub", "Sins", "CombSubFast")
SIGNAL_STEP, CTRL_STEP = 5, 4        # the fixture keeps signal[:, ::5] and ctrl[..., ::4] (a committed file stays small)


def weights():
    """(B, FR, 3) fp32: slot 0 ramps 1 -> 0, slot 1 ramps 0 -> 1, slot 2 is a sine of b + 1 periods around 0.5 - every row's
    own - scaled by 0.4; rows 1 and 2 run their ramps over a shorter stretch and then hold, so no two rows agree."""
    t = np.arange(FR, dtype=np.float64)
    w = np.zeros((B, FR, 3))
    for b in range(B):
        ramp = np.clip(t / (FR - 1 - 6 * b), 0.0, 1.0)
        w[b, :, 0] = 1.0 - ramp
        w[b, :, 1] = ramp
        w[b, :, 2] = 0.4 * (0.5 + 0.5 * np.sin(2 * np.pi * (b + 1) * t / FR))
    return w.astype(np.float32)
