"""Pitch correction (`ddsp_f0_tune`) stated in numpy fp64, and the cases of its kernel test.  include/ddsp_amd.h states the
same rule at the symbol; this file is the kernel's only yardstick.

THE RULE.  An owner's setting: mask (bit p in 0..11 allows pitch class p, C = 0; no bit: off), a4 Hz, strength s in [0, 1],
alpha in (0, 1].  A frame is voiced when its f0 is finite and > 0.  For the frames t < n of a row, in fp64:
    m_t = 69 + 12 * log2(f_t / a4)
    n_t = the integer n with bit (n mod 12) of mask set that minimises |n - m_t|; a tie takes the smaller n
    d_t = n_t - m_t                                   (0 where m_t is not finite)
    c_t = d_t                                         t is the row's first voiced frame, or frame t-1 is unvoiced   (reset)
    c_t = (1 - alpha) * c_(t-1) + alpha * d_t         otherwise
    out_t = (s * c_t == 0) ? f_t : (float)((double)f_t * exp2(s * c_t / 12))
Unvoiced frames, frames at or past the count, rows whose owner is off (no bit of the mask, or s == 0) or outside [0, J) keep
their bits.  A setting with a mask and a bad a4, s or alpha leaves its rows and raises the error word."""
import numpy as np


def offset(f, a4, mask):
    """d_t of one voiced frame: (d, m).  The sixteen integers around m ascend, and argmin keeps the first of a tie."""
    m = 69.0 + 12.0 * np.log2(np.float64(f) / np.float64(a4))
    if not np.isfinite(m):
        return 0.0, m
    base = int(np.floor(m))
    cand = [n for n in range(base - 7, base + 9) if (int(mask) >> (n % 12)) & 1]
    dist = np.abs(np.array(cand, dtype=np.float64) - m)
    return float(np.float64(cand[int(np.argmin(dist))]) - m), m


def bad_setting(a4, s, alpha):
    return not (np.isfinite(a4) and a4 > 0) or not (0 <= s <= 1) or not (0 < alpha <= 1)


def tune_rows(f0, mask, param, n_frames=None, owner=None):
    """f0 (B, Fr) fp32, mask (J,), param (J, 3) fp64 -> (out (B, Fr) fp32, corr (B, Fr) fp64, error word raised)."""
    f0 = np.asarray(f0, dtype=np.float32)
    B, Fr = f0.shape
    J = len(mask)
    out, corr, err = f0.copy(), np.zeros((B, Fr), dtype=np.float64), False
    for b in range(B):
        j = b if owner is None else int(owner[b])
        if not 0 <= j < J or (int(mask[j]) & 0xfff) == 0:
            continue
        a4, s, alpha = (np.float64(v) for v in param[j])
        if bad_setting(a4, s, alpha):
            err = True
            continue
        if s == 0:
            continue
        n = Fr if n_frames is None else min(max(int(n_frames[b]), 1), Fr)
        c, after_voiced = np.float64(0.0), False
        for t in range(n):
            f = f0[b, t]
            if not (np.isfinite(f) and f > 0):
                after_voiced = False
                continue
            d = np.float64(offset(f, a4, int(mask[j]) & 0xfff)[0])
            c = (np.float64(1.0) - alpha) * c + alpha * d if after_voiced else d
            after_voiced = True
            corr[b, t] = c
            if s * c != 0:
                out[b, t] = np.float32(np.float64(f) * np.exp2(s * c / np.float64(12.0)))
    return out, corr, err


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def boundary_distance(m, mask):
    """Semitones from m to the nearest decision boundary of `mask`: the midpoints of neighbouring allowed notes."""
    base = int(np.floor(m))
    notes = [n for n in range(base - 13, base + 15) if (int(mask) >> (n % 12)) & 1]
    return min(abs(m - (lo + hi) / 2.0) for lo, hi in zip(notes, notes[1:]))


def m_is_robust(f, a4):
    """True when m_t comes out the same fp64 number from every log2 that is good to an ulp: from the double nearest the true
    log2 (taken in extended precision) and from both its neighbours.  Two correct implementations of log2 - numpy's and the
    device's - may differ by an ulp, and 69 + 12 * log2 then rounds to a different m for some third of all inputs; on a frame
    that passes this, they cannot."""
    r = np.float64(f) / np.float64(a4)
    mid = np.float64(np.log2(np.longdouble(r)))
    ms = {float(69.0 + 12.0 * L) for L in (np.nextafter(mid, -np.inf), mid, np.nextafter(mid, np.inf))}
    return len(ms) == 1


def ulps32(a, b):
    """|a - b| in units of the last place of fp32 (finite a, b of one sign)."""
    ia, ib = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64), np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


# ---- the kernel test's cases ------------------------------------------------------------------------------------------------------
B = 5
SHAPES = [1, 63, 64, 65, 130]
A_MINOR = sum(1 << p for p in (9, 11, 0, 2, 4, 5, 7))
G_B = (1 << 7) | (1 << 11)
# owners: 0 off (no mask), 1 hard tuning (alpha 1), 2 alpha 0.05 at a4 = 442 and s = 0.8, 3 a bad setting (given per test),
# 4 the exact-tie mask {G, B} at a4 = 440, 5 off by s == 0
MASKS = np.array([0, A_MINOR, 0xfff & ~(1 << 1), A_MINOR, G_B, A_MINOR], dtype=np.int32)
PARAMS = np.array([[440.0, 1.0, 0.5], [440.0, 1.0, 1.0], [442.0, 0.8, 0.05], [440.0, 1.0, 0.3], [440.0, 1.0, 0.25],
                   [440.0, 0.0, 0.5]], dtype=np.float64)
J = len(MASKS)
BAD = [(3, 0, np.nan), (3, 0, 0.0), (3, 0, -440.0), (3, 0, np.inf), (3, 1, 1.5), (3, 1, -0.1), (3, 2, 0.0), (3, 2, 1.25),
       (3, 2, np.nan)]
GAP_VALUES = np.array([0.0, -130.0, np.nan, np.inf], dtype=np.float32)


def rows(Fr, seed=0):
    """(f0 (B, Fr) fp32, gaps (B, Fr) bool): f0 log-uniform in [60, 1000] Hz, every voiced frame more than 1e-6 semitones from a
    decision boundary of EVERY mask in `MASKS`, and with an m_t at a4 = 440 - the alpha == 1 owner's, whose c is held bit for bit -
    that does not hang on the last bit of log2 (`m_is_robust`); redrawn until both hold, and asserted.  Unvoiced gaps at frames 0, 62..65 and the last
    frame among others, their values 0, a negative number, NaN and inf in turn."""
    rng = np.random.Generator(np.random.PCG64(1000 + 7 * Fr + seed))
    f0 = np.empty((B, Fr), dtype=np.float32)
    for b in range(B):
        for t in range(Fr):
            while True:
                f = np.float32(60.0 * (1000.0 / 60.0) ** rng.random())
                if m_is_robust(f, 440.0) and all(boundary_distance(offset(f, p[0], m)[1], m) > 1e-6 for m, p in zip(MASKS, PARAMS) if m):
                    break
            f0[b, t] = f
    gaps = np.zeros((B, Fr), dtype=bool)
    for b, at in enumerate(([0], [62, 63], [64], [63, 64, 65], [Fr - 1])):
        for t in at:
            if t < Fr:
                gaps[b, t] = True
    gaps |= rng.random((B, Fr)) < 0.08
    if Fr > 1:
        gaps[1, 0] = False                                            # a row that starts voiced, whatever the draw
    f0[gaps] = GAP_VALUES[np.arange(int(gaps.sum())) % 4]
    for b in range(B):
        for t in range(Fr):
            if not gaps[b, t]:
                assert m_is_robust(f0[b, t], 440.0)
                for m, p in zip(MASKS, PARAMS):
                    assert m == 0 or boundary_distance(offset(f0[b, t], p[0], m)[1], m) > 1e-6
    return f0, gaps


def counts(Fr):
    """Counts of the five rows: some below Fr, a count of 1, and the full row."""
    return np.array([Fr, max(1, Fr - 1), 1, max(1, (2 * Fr) // 3), Fr], dtype=np.int32)


# owner tables over the five rows: the four live settings; then -1, J and a repeat among them
OWNERS = [np.array([1, 2, 0, 5, 2], dtype=np.int32), np.array([-1, 1, J, 2, 1], dtype=np.int32)]
