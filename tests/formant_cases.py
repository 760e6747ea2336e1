"""The formant warp, stated in numpy (include/ddsp_amd.h at `ddsp_ctrl_warp`): the only yardstick of the kernel.
Every operation is an `np.float32` operation, rounded once; t == 0 SELECTS the input's value, so a factor of 1, every exact hit
and every clamped end return the input's bits (-0.0, inf and NaN included)."""
import numpy as np

F32 = np.float32


def factor(semitones):
    """2 ** (s / 12) as a Python float stored to fp32: `hipddsp.formant_factor`'s number where it is used."""
    return F32(2 ** (float(semitones) / 12))


def warp_segment(x, alpha, origin):
    """x (n,) fp32 -> the segment read at f / alpha, origin 0 (bin j at j * df) or 1 (column j is harmonic j + 1)."""
    x = np.asarray(x, dtype=F32)
    n, alpha, o = x.shape[0], F32(alpha), F32(origin)
    out = x.copy()
    if n == 1:
        return out
    with np.errstate(all="ignore"):
        j = np.arange(n, dtype=np.int64) + int(origin)
        p = (j.astype(F32) / alpha).astype(F32)                      # one rounded quotient
        p = (p - o).astype(F32)                                      # one rounded difference
        p = np.minimum(np.maximum(p, F32(0)), F32(n - 1))
        i0 = np.floor(p).astype(np.int64)
        i1 = np.minimum(i0 + 1, n - 1)
        t = (p - i0.astype(F32)).astype(F32)                         # exact
        d = (x[i1] - x[i0]).astype(F32)
        lerp = (x[i0] + (d * t).astype(F32)).astype(F32)
        out = np.where(t == 0, x[i0], lerp).astype(F32)              # t == 0 selects: the input's bits
    return out


def bad(alpha):
    return not (np.isfinite(alpha) and alpha > 0)


def warp_rows(ctrl, segments, factors, Fr, slot_of_row=None, n_frames=None):
    """The statement of `ddsp_ctrl_warp` on ctrl (rows, sum) -> (the warped copy, error flag).  factors: (rows,) a factor per
    frame, (B,) one per batch row, or (S,) behind slot_of_row (B,), whose entries outside [0, S) are padding rows (factor 1).
    n_frames (B,): frames at or past a row's count keep their bits.  A factor that is not finite or not > 0 leaves its row as it
    was and raises the flag."""
    ctrl = np.asarray(ctrl, dtype=F32)
    out, err = ctrl.copy(), False
    rows, B = ctrl.shape[0], ctrl.shape[0] // Fr
    factors = np.asarray(factors, dtype=F32).reshape(-1)
    for r in range(rows):
        b, fr = divmod(r, Fr)
        if n_frames is not None and fr >= min(max(int(n_frames[b]), 1), Fr):
            continue
        if slot_of_row is not None:
            s = int(slot_of_row[b])
            if not 0 <= s < factors.shape[0]:
                continue
            alpha = factors[s]
        else:
            alpha = factors[r] if factors.shape[0] == rows and Fr > 1 else factors[b]
        if bad(alpha):
            err = True
            continue
        for first, n, origin in segments:
            out[r, first:first + n] = warp_segment(ctrl[r, first:first + n], alpha, origin)
    return out, err


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
