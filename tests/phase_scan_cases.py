"""The cases, references and CPU restatements of tests/test_phase_scan_cases_host.py (CPU) and tests/test_gpu_phase_scan.py
(device): `ddsp_phase_scan` (csrc/phase_scan.hip) - the f0 upsampling, the fp64 phase integral, `phase_frames` and the combtooth.

References, all from oracle/dsp.py and built once per (case, init) (`functools.lru_cache`; nobody writes into them):
  f0_up   `frames_to_samples`, fp32: the device has to give these bits
  rot64   fp64 cumulative sum of f0_up.double() / sr (+ init.double() / 2 / pi), wrapped x - rint(x), NOT rounded: the truth
  rot32   `rotation_from_f0` with precise True and False, fp32
  comb64(rot, f0)   sinc in fp64 of sr * rot.double() / (f0 + 1e-3), the `+ 1e-3` in fp32 as the reference does it
  comb32(rot, f0)   `sinc_comb`
Both comb references take `rot`: fed with the DEVICE's rot they judge the comb evaluation alone, and a wrap that went the other
way at +-0.5 needs no mask.

f0 tracks (PCG64 of the case's seed):
  voiced  uniform 65..800 Hz
  gaps    voiced, then: row 0 gets its first and last frame zeroed (Fr >= 3) and a run of zero frames in the middle (Fr >= 5);
          row 1 is zero throughout; row 2 (row 0 where B < 3) gets one frame at 0.05 Hz (sinc arguments up to 4.3e5 there;
          the zero frames, where the denominator is the bare 1e-3, reach 2.2e7).  With Fr == 1 the three rows are voiced,
          zero and 0.05 Hz.
  high    uniform 1000..1600 Hz: the largest running sum per sample, for the train-mode rounding

Cases, (B, Fr, hop, track, seed, aligned) - the smallest that reach each branch:
  (3,    1,  512, gaps)    Fr == 1: the frame is its own successor; B * Fr = 3 takes the tail exit of a 4-wave block
  (2,   65,  512, voiced)  frame 64 is the first whose prefix loop has an item (lane 0 only); 130 frames: a half-filled block
  (1,  130,  512, voiced)  three trips of the prefix loop (lanes 0 and 1)
  (3,    9,  512, gaps)    zero frames and the gate through the 512 kernels; 27 frames: tail exit
  (2,    5,  256, gaps)    generic kernel, 4 samples per lane
  (3,    7,  128, gaps)    generic kernel, 2 samples per lane
  (1,    3, 1024, voiced)  generic kernel, 16 per lane: the NL bound
  (2,    4,   48, voiced)  lanes 48..63 idle
  (1,    6,  100, gaps)    hop not a power of two: the scale 6 / 600 is inexact; 2 per lane, lanes 50..63 idle
  (1,   70,    1, voiced)  one live lane per wave; the prefix runs over 69 one-sample frames
  (2,    3,  512, voiced, unaligned)  every output a view one float past a 16-byte boundary: the generic kernel at hop 512
  (1, 2600,  512, voiced)  1.3 M samples, an fp64 prefix over 2600 frames            } one init setting (with), comb_mode 1
  (2,   40,  512, high)    the largest |S| per sample, meant for the train mode      } only: `settings()`
Every other case runs precise and train mode, with and without a per-row initial phase (0.3, -2.0, 7.0 by row), comb_mode 0, 1, 2.

Tolerances, none of them taken from the device's output:
  f0_up, phase = fl32(2 pi) * rot, phase_frames = phase[:, ::hop]: bit-equal.
  precise rot: wrap-aware |rot - rot64| <= 2^-24 everywhere.  Rounding a value of [-0.5, 0.5] to fp32 costs at most 2^-26
    (2^-25 at the ends); the fp64 sum and the product with 1/sr in place of the quotient cost < 1e-10 below 2^24 samples.
  train-mode rot against rot32: the device sums in another order, so the fp64 sum can land on the other side of an fp32
    rounding boundary: at most one fp32 ulp of the largest |S| of the case, and at most 1e-4 of the samples differ by more than
    2^-24 (the cap of tests/test_gpu_dsp.py; below 10 000 samples that is none).  `train_rot_model` restates the kernel's order
    (frame sums, exclusive prefix, in-frame running sum) and the host test holds the references themselves to both conditions.
  comb: max|comb - comb64| <= K_COMB * max(E32, 2^-23), E32 = max|comb32 - comb64| of the same rot and f0, nothing excluded.
    `comb_model` restates the kernel's evaluation on the CPU; over every case, mode and init setting here (fed with the
    oracle's rot32, so no device is involved) its error is 0.51..1.12 x max(E32, 2^-23) (model 6.4e-8..1.7e-7, E32
    8.9e-8..1.8e-7); tests/test_phase_scan_cases_host.py prints the ratio and holds it under COMB_MODEL_RATIO = 1.25, the
    measured 1.12 rounded up to the next quarter.  K_COMB = 16 x COMB_MODEL_RATIO = 20: the 16 x that
    tests/test_gpu_dsp_stages.py gives a device that differs from the restated arithmetic by rounding only (here: v_rcp_f32
    twice where the model divides).  20 x 1.2e-7 = 2.4e-6, an eighth of the 2e-5 of tests/test_gpu_dsp.py; a neighbouring
    sample's f0 or rot shows at 1e-3 or more.
"""
import functools

import numpy as np
import torch

from oracle import dsp as O

SR = 44100
TWO_PI32 = float(np.float32(2 * np.pi))      # the kernel's two_pi_f
PI32 = np.float32(np.pi)                     # the kernel's pi_f
INIT = (0.3, -2.0, 7.0)                      # initial phase of row b: INIT[b % 3]
ROT_TOL = 2.0 ** -24
FLIP_CAP = 1e-4
COMB_FLOOR = 2.0 ** -23
COMB_MODEL_RATIO = 1.25                      # measured 0.51..1.12, see above
K_COMB = 16.0 * COMB_MODEL_RATIO

CASES = [
    # B,  Fr,  hop, track,   seed, aligned
    (3, 1, 512, "gaps", 101, True),
    (2, 65, 512, "voiced", 102, True),
    (1, 130, 512, "voiced", 103, True),
    (3, 9, 512, "gaps", 104, True),
    (2, 5, 256, "gaps", 105, True),
    (3, 7, 128, "gaps", 106, True),
    (1, 3, 1024, "voiced", 107, True),
    (2, 4, 48, "voiced", 108, True),
    (1, 6, 100, "gaps", 109, True),
    (1, 70, 1, "voiced", 110, True),
    (2, 3, 512, "voiced", 111, False),
    (1, 2600, 512, "voiced", 112, True),
    (2, 40, 512, "high", 113, True),
]
LONG_CASE, HIGH_CASE = CASES[11], CASES[12]
FULL_CASES = CASES[:11]


def case_id(c):
    return "B%d-Fr%d-hop%d-%s" % c[:4] + ("" if c[5] else "-unaligned")


def settings(case):
    """-> (init settings, comb modes) the case runs with; `precise` goes both ways for every case."""
    if case in (LONG_CASE, HIGH_CASE):
        return (True,), (1,)
    return (False, True), (0, 1, 2)


def runs(cases=None):
    """[(case, precise, with_init)] and their ids, for `pytest.mark.parametrize`."""
    out = [(c, p, w) for c in (cases or CASES) for p in (True, False) for w in settings(c)[0]]
    return out, ["%s-%s-%s" % (case_id(c), "precise" if p else "train", "init" if w else "noinit") for c, p, w in out]


# ---- inputs -------------------------------------------------------------------------------------------------------------
def f0_track(B, Fr, track, seed):
    """(B, Fr, 1) fp32 frames."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lo, hi = (1000.0, 1600.0) if track == "high" else (65.0, 800.0)
    f = rng.uniform(lo, hi, size=(B, Fr)).astype(np.float32)
    if track == "gaps":
        if Fr >= 3:
            f[0, 0] = f[0, -1] = 0.0
        if Fr >= 5:
            a = Fr // 3
            f[0, a:a + max(1, Fr // 4)] = 0.0
        if B >= 2:
            f[1, :] = 0.0
        f[B - 1 if B >= 3 else 0, Fr // 2] = 0.05
    return torch.from_numpy(f).unsqueeze(-1)


def init_phase(B):
    return torch.tensor([INIT[b % 3] for b in range(B)], dtype=torch.float32)


# ---- references ---------------------------------------------------------------------------------------------------------
def wrap_diff(a, b):
    """|a - b| in cycles, fp64, where a wrap at +-0.5 is the same phase."""
    d = a.double() - b.double()
    return (d - torch.round(d)).abs()


def rot64_of(f0_up, init):
    acc = torch.cumsum(f0_up.double() / SR, dim=1)
    if init is not None:
        acc = acc + init.reshape(-1, 1).double() / 2 / np.pi
    return acc - torch.round(acc)


def train_sum32(f0_up, init):
    """The running sum the train mode wraps, as the oracle forms it: fp32 increments, ATen's cumsum (an fp64 accumulator
    rounded to fp32 per element), the fp32 initial phase added in fp32.  Its largest magnitude sets the ulp of the case."""
    acc = torch.cumsum(f0_up / SR, dim=1)
    if init is not None:
        acc = acc + init.reshape(-1, 1) / 2 / np.pi
    return acc


def comb64(rot, f0_up):
    den = (f0_up + 1e-3).double()                 # the sum in fp32, then widened
    return torch.sinc(float(SR) * rot.double() / den)


def comb32(rot, f0_up, zero_unvoiced=False):
    return O.sinc_comb(rot, f0_up, SR, zero_unvoiced)


@functools.lru_cache(maxsize=None)
def case_ref(case, with_init):
    B, Fr, hop, track, seed, _ = case
    f0_frames = f0_track(B, Fr, track, seed)
    init = init_phase(B) if with_init else None
    f0_up = O.frames_to_samples(f0_frames, hop).squeeze(-1).contiguous()
    rot32 = {p: O.rotation_from_f0(f0_up, SR, init, p) for p in (True, False)}
    s32 = train_sum32(f0_up, init)
    return dict(B=B, Fr=Fr, hop=hop, T=Fr * hop, f0_frames=f0_frames, init=init, f0_up=f0_up, rot64=rot64_of(f0_up, init),
                rot32=rot32, ulp_S=float(np.spacing(np.float32(s32.abs().max()))))


def check_train_rot(what, rot, k):
    """The two train-mode conditions of the module docstring for `rot` against the oracle's rot32; -> (max, share)."""
    d = wrap_diff(rot, k["rot32"][False])
    worst, share = float(d.max()), float((d > ROT_TOL).double().mean())
    print(f"TRAIN {what}: max wrap-aware difference {worst:.3e} (one ulp of the largest |S|: {k['ulp_S']:.3e}), "
          f"share above 2^-24: {share:.3e} ({int((d > ROT_TOL).sum())} of {d.numel()})")
    assert worst <= k["ulp_S"], (what, "train-mode rot: max wrap-aware difference", worst, "one ulp of max|S|", k["ulp_S"])
    assert share <= FLIP_CAP, (what, "train-mode rot: share of samples beyond 2^-24", share, "cap", FLIP_CAP)
    return worst, share


# ---- CPU restatements of the kernel -----------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fl32(a * b + c) for fp32 arrays: the product is exact in fp64 and the sum rounds there once before the fp32 rounding."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def upsample_model(f0_frames, hop):
    """The kernel's upsampling: src = fl32(scale * t), w1 = src - m with m = t // hop (not floor(src)), x1 clamped at the
    last frame, out = fma(1 - w1, x0, fl32(w1 * x1)).  (B, Fr, 1) -> (B, Fr * hop) fp32."""
    x = f0_frames.squeeze(-1).numpy()
    B, Fr = x.shape
    scale = np.float32(Fr) / np.float32(Fr * hop)
    t = np.arange(Fr * hop)
    m = t // hop
    src = scale * t.astype(np.float32)
    w1 = src - m.astype(np.float32)
    x0, x1 = x[:, m], x[:, np.minimum(m + 1, Fr - 1)]
    w1b = np.broadcast_to(w1, x0.shape)
    return torch.from_numpy(_fma32(np.float32(1.0) - w1b, x0, w1b * x1))


def train_rot_model(f0_up, init, hop):
    """The kernel's train-mode summation order: fp64 frame sums of the fp32 increments, their exclusive prefix along the row,
    the running sum inside the frame; S = prefix + running rounded to fp32, the fp32 initial phase added in fp32, wrapped."""
    inc = (f0_up.numpy() / np.float32(SR)).astype(np.float64)
    B, T = inc.shape
    run = np.cumsum(inc.reshape(B, T // hop, hop), axis=2)
    fsum = run[:, :, -1]
    before = np.concatenate([np.zeros((B, 1)), np.cumsum(fsum, axis=1)[:, :-1]], axis=1)
    s = (before[:, :, None] + run).reshape(B, T).astype(np.float32)
    if init is not None:
        s = s + ((init.numpy() / np.float32(2.0)) / PI32)[:, None]
    return torch.from_numpy(s - np.rint(s))


def comb_model(rot, f0_up):
    """The kernel's comb in fp32 numpy: quotient (correctly rounded here, within 1 ulp there), the exact reduction
    x - 2 rint(x / 2), the fold to [-0.5, 0.5], the odd polynomial to t^13, sin / (fl32(pi) * x) by reciprocal and product."""
    one, two, half = np.float32(1.0), np.float32(2.0), np.float32(0.5)
    r, f = rot.numpy(), f0_up.numpy()
    x = (np.float32(SR) * r) / (f + np.float32(1e-3))
    xr = _fma32(np.full_like(x, -two), np.rint(half * x), x)
    t = np.where(np.abs(xr) > half, np.copysign(one, xr) - xr, xr)
    t2 = t * t
    pl = np.full_like(t, np.float32(0.00046630281))
    for c in (-0.0073704309, 0.082145887, -0.59926453, 2.5501640, -5.1677128, 3.1415927):
        pl = _fma32(pl, t2, np.full_like(t, np.float32(c)))
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (t * pl) * (one / (PI32 * x))
    return torch.from_numpy(np.where(x == 0, one, c).astype(np.float32))
