"""The key timeline rule as an fp64 numpy statement, and the tables the kernels take - written from include/ddsp_amd.h alone,
with nothing of the package imported: the tests hold `ddsp_pieces_gather_keys` and `ddsp_bank_key_glide` to THIS.

A timeline is n >= 1 breakpoints (time, semitones), times strictly increasing.  The key at tau is linear in semitones between
two breakpoints, the first one's before them, the last one's after them; the f0 factor is 2 ** (key / 12).  Every breakpoint
carries its semitones (fp32) and a STORED factor, 2 ** (float(key) / 12) as a Python float stored to fp32.  The stored factor is
the answer where no slope is at work:
  (a) tau before the first breakpoint  -> the first one's,
  (b) tau behind the last              -> the last one's,
  (c) tau exactly on a breakpoint      -> its own,
  (d) between two of equal semitones   -> the earlier one's.
Elsewhere the factor is fp32(exp2((s0 + (s1 - s0) * ((tau - t0) / (t1 - t0))) / 12.0)) with every step in fp64."""
import numpy as np


def stored_factor(key):
    """The factor the host forms for a constant key: 2 ** (float(key) / 12), a Python float, stored to fp32."""
    return np.float32(2 ** (float(key) / 12))


def factors(times, semi, fac, taus):
    """The rule -> (factor (len(taus),) fp32, stored (len(taus),) bool: True where one of the cases (a)-(d) gave a stored factor).
    times: the breakpoint times, strictly increasing; semi, fac: fp32 semitones and stored factors; taus: fp64 times."""
    times = np.asarray(times, dtype=np.float64)
    semi, fac = np.asarray(semi, dtype=np.float32), np.asarray(fac, dtype=np.float32)
    n = len(times)
    out, stored = np.zeros(len(taus), dtype=np.float32), np.zeros(len(taus), dtype=bool)
    for i, tau in enumerate(np.asarray(taus, dtype=np.float64)):
        p = int(np.searchsorted(times, tau, side="right"))               # the first breakpoint behind tau
        if p == 0:                                                       # (a)
            out[i], stored[i] = fac[0], True
        elif p == n:                                                     # (b), and (c) for the last breakpoint
            out[i], stored[i] = fac[n - 1], True
        elif tau == times[p - 1] or semi[p - 1] == semi[p]:              # (c), (d)
            out[i], stored[i] = fac[p - 1], True
        else:
            t0, t1 = times[p - 1], times[p]
            s0, s1 = np.float64(semi[p - 1]), np.float64(semi[p])
            out[i] = np.float32(np.exp2((s0 + (s1 - s0) * ((tau - t0) / (t1 - t0))) / np.float64(12.0)))
    return out, stored


def tables(jobs):
    """jobs: per job a number of semitones (one breakpoint at frame 0) or a list of (frame, semitones) -> the numpy tables of
    `ddsp_pieces_gather_keys`: (bp_off (J + 1,) int32, bp_frame (P,) int32, bp_semi (P,) fp32, bp_fac (P,) fp32)."""
    off, frame, semi, fac = [0], [], [], []
    for job in jobs:
        for at, key in ([(0, job)] if np.isscalar(job) else job):
            frame.append(int(at))
            semi.append(float(key))
            fac.append(stored_factor(key))
        off.append(len(frame))
    return (np.array(off, dtype=np.int32), np.array(frame, dtype=np.int32), np.array(semi, dtype=np.float32),
            np.array(fac, dtype=np.float32))


def gather_f0(f0, n_file_frames, rows, tabs, N_max):
    """The f0 rows of `ddsp_pieces_gather_keys` -> (f0_rows (R, N_max) fp32, stored (R, N_max) bool, bad (R,) bool).  f0 (F, Fr_max)
    fp32; rows (R, 6) (file, start_frame, n_frames, start_sample, n_samples, job).  Frame t < n_frames is fp32(f0) * factor at
    file frame start_frame + t, ONE rounded fp32 product; zeros behind.  A row whose file, frames, job or breakpoint range is out
    of bounds is all zeros and `bad`."""
    bp_off, bp_frame, bp_semi, bp_fac = tabs
    J, P, F = len(bp_off) - 1, len(bp_frame), f0.shape[0]
    out = np.zeros((len(rows), N_max), dtype=np.float32)
    stored, bad = np.zeros((len(rows), N_max), dtype=bool), np.zeros(len(rows), dtype=bool)
    for r, (file, sf, nf, _, _, job) in enumerate(rows):
        ok = 0 <= file < F and 0 <= job < J and sf >= 0 and nf >= 0 and nf <= N_max
        ok = ok and sf + nf <= n_file_frames[file]
        if ok:
            lo, hi = int(bp_off[job]), int(bp_off[job + 1])
            ok = lo >= 0 and hi > lo and hi <= P
        if not ok:
            bad[r] = True
            continue
        k, stored[r, :nf] = factors(bp_frame[lo:hi], bp_semi[lo:hi], bp_fac[lo:hi], np.arange(sf, sf + nf, dtype=np.float64))
        out[r, :nf] = f0[file, sf:sf + nf].astype(np.float32) * k            # fp32 * fp32 in numpy: one rounded product
    return out, stored, bad


def bank_pitch_frames(rows, W, clock, key_n, key_t, key_semi, key_fac, pitch, Fr, n_in, block, hop):
    """The statement of `ddsp_bank_key_glide` -> (pitch_frames (W, Fr) fp32, stored (W, Fr) bool, the clocks after the call).  A row
    whose slot lies outside [0, S) is padding: 1.0 in every frame, no clock touched.  For a real row c = clock[s] + block, frame
    t has tau = float64(c - n_in) + t * hop; with key_n[s] == 0 every frame gets pitch[s]; then clock[s] = c."""
    clock = np.array(clock, dtype=np.int64)
    S, P_max = np.asarray(key_t).shape
    out, stored = np.ones((int(W), int(Fr)), dtype=np.float32), np.ones((int(W), int(Fr)), dtype=bool)
    for r in range(int(W)):
        s = r if rows is None else int(rows[r])
        if not 0 <= s < S:
            continue
        c = int(clock[s]) + int(block)
        n = min(max(int(key_n[s]), 0), P_max)
        if n == 0:
            out[r] = np.float32(pitch[s])
        else:
            taus = np.float64(c - int(n_in)) + np.arange(int(Fr), dtype=np.float64) * np.float64(hop)
            out[r], stored[r] = factors(key_t[s, :n], key_semi[s, :n], key_fac[s, :n], taus)
        clock[s] = c
    return out, stored, clock


def ulps(got, want):
    """|got - want| in units of the fp32 spacing at `want` -> fp64 array."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
