"""numpy restatement of the autocorrelation f0 extractor behind `F0_Extractor('ac')` (Boersma 1993, with the parameters
of the reference's `'parselmouth'` call) and the seeded signals its tests share.

`dtype` is the precision of the signal path - the row statistics, the windowed frame, the FFT autocorrelation and its
normalisation.  The candidate refinement (sinc interpolation, Brent) and the path search run in fp64 under either dtype, as
they do in the kernels; frame geometry is fp64 arithmetic on integers under either.  `dtype=np.float32` is therefore the
kernel's precision split with numpy's FFT summation order, `dtype=np.float64` the reference for the tests."""
import math

import numpy as np

VOICING, SILENCE, OCTAVE, OCTAVE_JUMP, VUV = 0.6, 0.03, 0.01, 0.35, 0.14
GEOMETRIES = {            # name: (sample rate, hop, f0_min, f0_max)
    "16k": (16000, 160, 65, 800),
    "44k": (44100, 512, 65, 800),
    "48k": (48000, 480, 50, 1100),
}


def geometry(sr, f0_min, f0_max):
    dx = 1.0 / sr
    w0 = int(math.floor(3.0 / f0_min / dx))
    half = w0 // 2 - 1
    W = 2 * half
    nfft = 1
    while nfft < 1.5 * W:
        nfft *= 2
    period = int(math.floor(sr / f0_min))
    return dict(W=W, half=half, nfft=nfft, imax=W // 2, lag_min=max(2, int(math.floor(sr / f0_max))),
                lag_max=min(W // 3 + 2, W), period=period, half_period=period // 2 + 1,
                C=max(15, int(math.floor(f0_max / f0_min))))


def ac_frames(N, sr, hop, f0_min):
    """Frames of an N-sample row (0 or less: the row is shorter than one window)."""
    dx, dt = 1.0 / sr, hop / sr
    return int(math.floor((N * dx - 3.0 / f0_min) / dt)) + 1


def min_samples(sr, hop, f0_min):
    n = int(3.0 / f0_min * sr) - 2
    while ac_frames(n, sr, hop, f0_min) < 1:
        n += 1
    return n


def frame_left(N, nF, i, sr, hop):
    dx, dt = 1.0 / sr, hop / sr
    t = 0.5 * N * dx - 0.5 * nF * dt + 0.5 * dt + i * dt
    return int(math.floor(t / dx - 0.5))


def pad_frames(N, nF, hop, start_frame=0):
    return start_frame + (int(N // hop) - nF + 1) // 2


def window(W):
    j = np.arange(W, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (j + 1.0) / (W + 1.0))


def window_ac(W, nfft, imax):
    h = window(W)
    a = np.fft.irfft(np.abs(np.fft.rfft(h, nfft)) ** 2, nfft)
    return a[:imax + 1] / a[0]


def sinc_interp(r, imax, x, depth):
    """Hann-windowed sinc interpolation of the even sequence r[|k|], |k| <= imax, at x (fp64)."""
    m = int(math.floor(x))
    if x == m:
        return float(r[abs(m)])
    D = min(depth, m + imax + 1, imax - m)
    L, R = m + 1 - D, m + D
    kl = np.arange(L, m + 1)
    kr = np.arange(m + 1, R + 1)
    ul, ur = x - kl, kr - x
    left = r[np.abs(kl)] * (np.sin(np.pi * ul) / (np.pi * ul)) * (0.5 + 0.5 * np.cos(np.pi * ul / (x - L + 1)))
    right = r[np.abs(kr)] * (np.sin(np.pi * ur) / (np.pi * ur)) * (0.5 + 0.5 * np.cos(np.pi * ur / (R - x + 1)))
    return float(np.sum(left) + np.sum(right))


def brent_max(f, a, b, tol=1e-10, itermax=60):
    """Brent's minimiser (golden section + parabolic steps) on -f over [a, b]; returns (x, f(x))."""
    golden = 1.0 - 0.6180339887498948482045868343656381177203
    sqrt_eps = math.sqrt(np.finfo(np.float64).eps)
    v = a + golden * (b - a)
    fv = -f(v)
    x = w = v
    fx = fw = fv
    for _ in range(itermax):
        rng = b - a
        mid = 0.5 * (a + b)
        tol_act = sqrt_eps * abs(x) + tol / 3.0
        if abs(x - mid) + 0.5 * rng <= 2.0 * tol_act:
            break
        step = golden * ((b - x) if x < mid else (a - x))
        if abs(x - w) >= tol_act:
            t = (x - w) * (fx - fv)
            q = (x - v) * (fx - fw)
            p = (x - v) * q - (x - w) * t
            q = 2.0 * (q - t)
            if q > 0.0:
                p = -p
            else:
                q = -q
            if abs(p) < abs(step * q) and p > q * (a - x + 2.0 * tol_act) and p < q * (b - x - 2.0 * tol_act):
                step = p / q
        if abs(step) < tol_act:
            step = tol_act if step > 0.0 else -tol_act
        t = x + step
        ft = -f(t)
        if ft <= fx:
            if t < x:
                b = x
            else:
                a = x
            v, w, x = w, x, t
            fv, fw, fx = fw, fx, ft
        else:
            if t < x:
                a = t
            else:
                b = t
            if ft <= fw or w == x:
                v, w = w, t
                fv, fw = fw, ft
            elif ft <= fv or v == x or v == w:
                v, fv = t, ft
    return x, -fx


def frame_candidates(x, mean, left, g, hw, sr, f0_min, f0_max, dtype):
    """One frame: (freq (C,), strength (C,), n candidates, lpeak); candidate 0 is the unvoiced one."""
    W, half, nfft, imax = g["W"], g["half"], g["nfft"], g["imax"]
    N = x.shape[0]
    right = left + 1
    xm = x - mean                                       # dtype
    lmean = xm[right - g["period"]:left + g["period"] + 1].mean(dtype=dtype)
    lo, hi = max(0, left - g["half_period"]), min(N - 1, right + g["half_period"])
    lpeak = float(np.max(np.abs(xm[lo:hi + 1] - lmean)))
    f = (xm[right - half:right - half + W] - lmean) * window(W).astype(dtype)
    a = np.fft.irfft(np.abs(np.fft.rfft(f, nfft)) ** 2, nfft)
    C = g["C"]
    freq, stren, lag = np.zeros(C), np.zeros(C), np.zeros(C, dtype=np.int64)
    n = 1
    if lpeak == 0.0 or not a[0] > 0:
        return freq, stren, n, lpeak
    assert a.dtype == dtype
    r = (a[:imax + 1] / (a[0] * hw.astype(dtype))).astype(np.float64)
    for l in range(g["lag_min"], g["lag_max"]):
        if not (l < imax and r[l] > 0.5 * VOICING and r[l] > r[l - 1] and r[l] >= r[l + 1]):
            continue
        den = 2.0 * r[l] - r[l - 1] - r[l + 1]
        if not (den > 0.0 and math.isfinite(den)):      # a frame of rounding residue only (digital silence)
            continue
        tau = l + 0.5 * (r[l + 1] - r[l - 1]) / den
        fq = sr / tau
        s = sinc_interp(r, imax, tau, 30)
        if s > 1.0:
            s = 1.0 / s
        if not (fq < f0_max and math.isfinite(s)):
            continue
        if n < C:
            place = n
            n += 1
        else:
            weakest, place = 2.0, -1
            for k in range(1, C):
                ls = stren[k] - OCTAVE * math.log2(f0_min / freq[k])
                if ls < weakest:
                    weakest, place = ls, k
            if s - OCTAVE * math.log2(f0_min / fq) <= weakest:
                place = -1
        if place >= 0:
            freq[place], stren[place], lag[place] = fq, s, l
    for k in range(1, n):
        tau, s = brent_max(lambda t: sinc_interp(r, imax, t, 70), lag[k] - 1.0, lag[k] + 1.0)
        if s > 1.0:
            s = 1.0 / s
        freq[k], stren[k] = sr / tau, s
    return freq, stren, n, lpeak


def viterbi(freq, stren, ncand, lpeak, gpeak, sr, hop, f0_max):
    """The best path: chosen candidate per frame (ties to the lower index)."""
    nF, C = freq.shape
    dt = hop / sr
    corr = 0.01 / dt
    oj, vu = OCTAVE_JUMP * corr, VUV * corr
    voiced = freq > 0
    lf = np.where(voiced, np.log2(np.where(voiced, freq, 1.0)), 0.0)
    inten = np.minimum(1.0, lpeak / gpeak) if gpeak > 0 else np.zeros(nF)
    unv = VOICING + np.maximum(0.0, 2.0 - inten / (SILENCE / (1.0 + VOICING)))
    score = np.where(voiced, stren - OCTAVE * (math.log2(f0_max) - lf), unv[:, None])
    valid = np.arange(C)[None, :] < np.asarray(ncand)[:, None]
    delta = np.where(valid[0], score[0], -np.inf)
    psi = np.zeros((nF, C), dtype=np.int64)
    for i in range(1, nF):
        cost = np.where(voiced[i - 1][:, None] & voiced[i][None, :], oj * np.abs(lf[i - 1][:, None] - lf[i][None, :]),
                        np.where(voiced[i - 1][:, None] | voiced[i][None, :], vu, 0.0))
        tot = np.where(valid[i - 1][:, None], delta[:, None] - cost, -np.inf)
        psi[i] = np.argmax(tot, axis=0)                  # first maximum: the lower index
        delta = np.where(valid[i], tot[psi[i], np.arange(C)] + score[i], -np.inf)
    path = np.zeros(nF, dtype=np.int64)
    path[-1] = int(np.argmax(delta))
    for i in range(nF - 1, 0, -1):
        path[i - 1] = psi[i, path[i]]
    return path


def analyse(x, sr, hop, f0_min, f0_max, dtype=np.float64):
    """x (N,) -> dict(f0 (nF,), choice (nF,), freq / stren (nF, C), ncand, lpeak, gpeak)."""
    g = geometry(sr, f0_min, f0_max)
    x = np.asarray(x, dtype=dtype)
    N = x.shape[0]
    nF = ac_frames(N, sr, hop, f0_min)
    if nF < 1:
        raise ValueError("row shorter than one analysis window")
    hw = window_ac(g["W"], g["nfft"], g["imax"])
    mean = x.mean(dtype=np.float64).astype(dtype)
    gpeak = float(np.max(np.abs(x - mean)))
    C = g["C"]
    freq, stren, ncand, lpeak = np.zeros((nF, C)), np.zeros((nF, C)), np.ones(nF, dtype=np.int64), np.zeros(nF)
    if gpeak > 0:
        for i in range(nF):
            freq[i], stren[i], ncand[i], lpeak[i] = frame_candidates(x, mean, frame_left(N, nF, i, sr, hop), g, hw, sr, f0_min,
                                                                     f0_max, dtype)
    path = viterbi(freq, stren, ncand, lpeak, gpeak, sr, hop, f0_max)
    f0 = freq[np.arange(nF), path]
    return dict(f0=f0, choice=path, freq=freq, stren=stren, ncand=ncand, lpeak=lpeak, gpeak=gpeak)


def uv_interp_clamp(f0, f0_min):
    f0 = np.array(f0, dtype=np.float64)
    uv = f0 == 0
    if len(f0[~uv]) > 0:
        f0[uv] = np.interp(np.where(uv)[0], np.where(~uv)[0], f0[~uv])
    f0[f0 < f0_min] = f0_min
    return f0


def extract(x, sr, hop, f0_min, f0_max, uv_interp=False, silence_front=0, dtype=np.float64):
    """The wrapper: crop, analyse, pad to N // hop + 1 frames, optionally interpolate over unvoiced frames and clamp."""
    x = np.asarray(x)
    n_frames = int(len(x) // hop) + 1
    start_frame = int(silence_front * sr / hop)
    xc = x[int(np.round(start_frame * hop / sr * sr)):]
    raw = analyse(xc, sr, hop, f0_min, f0_max, dtype)["f0"]
    pad = pad_frames(len(xc), len(raw), hop, start_frame)
    f0 = np.zeros(n_frames)
    f0[pad:pad + len(raw)] = raw
    return uv_interp_clamp(f0, f0_min) if uv_interp else f0


# ---- signals (seeded; amplitudes well above the silence threshold unless said) ----------------------------------------------
def harmonic_tone(sr, dur, f0, seed=0, partials=8):
    t = np.arange(int(round(sr * dur))) / sr
    rng = np.random.default_rng(seed)
    x = np.zeros_like(t)
    for k in range(1, partials + 1):
        x += np.sin(2 * np.pi * k * f0 * t + rng.uniform(0, 2 * np.pi)) / k
    return (0.3 * x / np.max(np.abs(x))).astype(np.float32)


def glide(sr, dur, f_lo=80.0, f_hi=600.0, partials=4):
    """Exponential glide; returns (signal, instantaneous f0 per sample)."""
    t = np.arange(int(round(sr * dur))) / sr
    f = f_lo * (f_hi / f_lo) ** (t / dur)
    ph = 2 * np.pi * np.cumsum(f) / sr
    x = sum(np.sin(k * ph) / k for k in range(1, partials + 1))
    return (0.3 * x / np.max(np.abs(x))).astype(np.float32), f


def segments(sr, dur, f0=220.0, seed=1):
    """tone / silence / white noise / tone, a quarter of `dur` each."""
    n = int(round(sr * dur))
    q = n // 4
    rng = np.random.default_rng(seed)
    x = np.zeros(n)
    tone = harmonic_tone(sr, dur, f0, seed).astype(np.float64)
    x[:q] = tone[:q]
    x[2 * q:3 * q] = 0.2 * rng.standard_normal(q)
    x[3 * q:] = tone[3 * q:]
    return x.astype(np.float32)


def zeros(sr, dur):
    return np.zeros(int(round(sr * dur)), dtype=np.float32)


def octave_trap(sr, dur, f0=110.0):
    """A tone at f0 whose second harmonic is the stronger partial."""
    t = np.arange(int(round(sr * dur))) / sr
    x = 0.5 * np.sin(2 * np.pi * f0 * t) + 1.0 * np.sin(2 * np.pi * 2 * f0 * t + 0.7) + 0.3 * np.sin(2 * np.pi * 3 * f0 * t + 1.9)
    return (0.3 * x / np.max(np.abs(x))).astype(np.float32)


def signals(sr, dur):
    """{name: (signal, ground-truth f0 per sample or None)}"""
    g, gf = glide(sr, dur)
    return {
        # (not 196 Hz: its period is exactly 225 samples at 44.1 kHz, and the depth-70 interpolant, which changes its set of
        # samples at every integer lag, then has two maxima of equal height 0.0009 samples to either side of the lag)
        "tone": (harmonic_tone(sr, dur, 190.7), np.full(int(round(sr * dur)), 190.7)),
        "glide": (g, gf),
        "segments": (segments(sr, dur), None),
        "octave": (octave_trap(sr, dur), np.full(int(round(sr * dur)), 110.0)),
    }
