"""The cases, float64 / float32 references and generator restatements of tests/test_dsp_stage_cases_host.py (CPU) and
tests/test_gpu_dsp_stages.py (device): the sinusoid bank (csrc/sins_bank.hip), the spectral overlap-add
(csrc/spectral_ola.hip) and the two in-kernel noise generators.

Every reference is evaluated twice from the same fp32 inputs: in float64 (`y64`, `d64`: the truth) and in float32 (`y32`,
`d32`: what the oracle itself gives at the device's precision).  The distance of the two is the reference's own error,

    E32 = ||x32 - x64|| / ||x64||    (`rel_err`),        max|x32 - x64|    (`max_err`),

and the device tests bound the device's error by a multiple of it.  A case is built once (`functools.lru_cache`) and shared:
nobody writes into what `bank_case` / `ola_case` return.

Bank cases, (B, Fr, H, hop, col0, seed) - the smallest that reach each branch of the two entry points:
  (2, 3, 150,  512)        scalar forward (H % 4 != 0); generic backward
  (1, 2, 100,  512)        packed forward; generic backward
  (2, 3,  37, 1024)        scalar forward (hop != 512); generic backward with 4 samples per lane
  (1, 4, 256,  256)        scalar forward; partial32 with its second sample slot empty
  (2, 5,  96,   64)        partial32 with most lanes idle
  (1, 1, 128,  512)        Fr == 1: the frame is its own successor, forward and backward
  (1, 3,  33,  512) col0=3 one harmonic past a re-seed block; a control block at an odd column (scalar loads)
  (1, 2,   1,  512)        H = 1
OLA cases, (B, Fr, seed, comb): (2, 1) is the backward's double pass on frame 0 (m0 == Fr - 1 == 0 folds frames 0 and 1
into one workgroup); (1, 5) takes its comb from `sinc_comb` of an f0 track, the others a uniform one.
"""
import functools

import numpy as np
import torch

from oracle import dsp as O

SR = 44100
FMAX = SR / 2
NB = 513                      # bins of one OLA control block
OLA_HOP = 512
PI32 = float(np.float32(np.pi))   # the kernel's pi_f

BANK_CASES = [
    # B, Fr,  H,  hop, col0, seed
    (2, 3, 150, 512, 4, 11),
    (1, 2, 100, 512, 4, 12),
    (2, 3, 37, 1024, 4, 13),
    (1, 4, 256, 256, 4, 47),
    (2, 5, 96, 64, 4, 15),
    (1, 1, 128, 512, 4, 16),
    (1, 3, 33, 512, 3, 17),
    (1, 2, 1, 512, 4, 45),
]
LDS_RANGE_CASE = (1, 1, 2048, 512, 19)     # (B, Fr, H, hop, seed): the last H the generic backward's LDS holds; partial32 takes it
OLA_CASES = [
    # B, Fr, seed, comb
    (2, 1, 21, "uniform"),
    (2, 2, 22, "uniform"),
    (1, 5, 23, "sinc"),
    (3, 9, 24, "uniform"),
]


def bank_id(c):
    return "B%d-Fr%d-H%d-hop%d-col%d" % c[:5]


def ola_id(c):
    return "B%d-Fr%d-%s" % (c[0], c[1], c[3])


def rel_err(x, x64):
    """||x - x64|| / ||x64|| in float64."""
    return float((x.double() - x64).norm() / x64.norm())


def max_err(x, x64):
    return float((x.double() - x64).abs().max())


# ---- sinusoid bank ------------------------------------------------------------------------------------------------------
def bank_keep(f0_frames, H):
    """remove_above_fmax as the kernel forms it, all in fp32: (fp32(f0 * k) < fmax) + 1e-7, k = 1..H.  (B, Fr, H) fp32."""
    k = torch.arange(1, H + 1, dtype=torch.float32)
    return (f0_frames * k < FMAX).float() + 1e-7


def bank_phase(f0_frames, hop):
    """(B, Fr*hop) fp32 radians: the fp64-integrated wrapped rotation of the upsampled f0, rounded once."""
    f0 = O.frames_to_samples(f0_frames, hop).squeeze(-1)
    return (2 * np.pi * O.rotation_from_f0(f0, SR, None, True)).float()


def bank_reference(ctrl, col0, H, f0_frames, phase, g, hop, dtype):
    """-> (y (B, T), d (B, Fr, H)) in `dtype`: the bank and the gradient of (y * g).sum() w.r.t. its control block."""
    c = ctrl[..., col0:col0 + H].to(dtype).clone().requires_grad_(True)
    keep = bank_keep(f0_frames, H).to(dtype)          # fp32 values, cast
    y = O.harmonic_bank(torch.exp(c) / 128 * keep, phase.to(dtype), hop)
    (y * g.to(dtype)).sum().backward()
    return y.detach(), c.grad.detach()


@functools.lru_cache(maxsize=None)
def bank_case(B, Fr, H, hop, seed, col0=4):
    rng = np.random.Generator(np.random.PCG64(seed))
    ctrl = torch.from_numpy((rng.standard_normal((B, Fr, H + 8)) * 0.5).astype(np.float32))
    f0_frames = torch.from_numpy(rng.uniform(65, 800, (B, Fr, 1)).astype(np.float32))
    f0_frames[0, 0] = 441.0      # 441 * 50 == 22050.0 == fmax exactly in fp32: `<` is strict, harmonic 50 is masked
    phase = bank_phase(f0_frames, hop)
    g = torch.from_numpy(rng.standard_normal((B, Fr * hop)).astype(np.float32))
    y64, d64 = bank_reference(ctrl, col0, H, f0_frames, phase, g, hop, torch.float64)
    y32, d32 = bank_reference(ctrl, col0, H, f0_frames, phase, g, hop, torch.float32)
    masked = bank_keep(f0_frames, H) < 0.5            # (B, Fr, H) bool
    return dict(B=B, Fr=Fr, H=H, hop=hop, col0=col0, ctrl=ctrl, f0_frames=f0_frames, phase=phase, g=g, masked=masked,
                y64=y64, y32=y32, d64=d64, d32=d32)


# ---- spectral overlap-add -----------------------------------------------------------------------------------------------
def ola_reference(ctrl, comb, u, g, B, Fr, dtype):
    """-> (y (B, T), d (B*Fr, 3*513)) in `dtype`: the OLA and the gradient of (y * g).sum() w.r.t. the three blocks."""
    c = ctrl[:, :3 * NB].to(dtype).clone().requires_grad_(True)
    hm, hp, nm = (c[:, i * NB:(i + 1) * NB].reshape(B, Fr, NB) for i in range(3))
    noise = (2 * u - 1).to(dtype)                      # exact in fp32: u is on the 24-bit grid
    y = O.windowed_spectral_ola(comb.to(dtype), noise, torch.exp(hm + 1j * PI32 * hp), torch.exp(nm) / 128, OLA_HOP)
    (y * g.to(dtype)).sum().backward()
    return y.detach(), c.grad.detach()


@functools.lru_cache(maxsize=None)
def ola_case(B, Fr, seed, comb="uniform"):
    rng = np.random.Generator(np.random.PCG64(seed))
    T = Fr * OLA_HOP
    ctrl = torch.from_numpy((rng.standard_normal((B * Fr, 3 * NB + 5)) * 0.5).astype(np.float32))   # stride wider than the blocks
    if comb == "sinc":
        import synthetic
        f0_frames = synthetic.make_inputs(seed, B, Fr, with_noise=False)["f0"]
        f0 = O.frames_to_samples(f0_frames, OLA_HOP).squeeze(-1)
        cmb = O.sinc_comb(O.rotation_from_f0(f0, SR, None, True), f0, SR)
    else:
        cmb = torch.from_numpy(rng.uniform(-1, 1, (B, T)).astype(np.float32))
    u = torch.from_numpy(rng.random((B, T), dtype=np.float32))
    g = torch.from_numpy(rng.standard_normal((B, T)).astype(np.float32))
    y64, d64 = ola_reference(ctrl, cmb, u, g, B, Fr, torch.float64)
    y32, d32 = ola_reference(ctrl, cmb, u, g, B, Fr, torch.float32)
    return dict(B=B, Fr=Fr, ctrl=ctrl, comb=cmb, u=u, g=g, y64=y64, y32=y32, d64=d64, d32=d32)


OLA_BLOCKS = {"hm": slice(0, NB), "hp": slice(NB, 2 * NB), "nm": slice(2 * NB, 3 * NB)}


# ---- the two in-kernel generators, as exact integer arithmetic ------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def _index(B, T):
    return np.arange(B * T, dtype=np.uint64)          # b * T + t


def _unit(v24, B, T):
    return (v24.astype(np.float32) / np.float32(16777216.0)).reshape(B, T)


def unit_noise_fir(seed, B, T):
    """`ddsp_hash32` (csrc/common.h) of (seed, b*T + t), top 24 bits / 2**24: the draw of ltv_fir.hip and ragged.hip."""
    seed = int(seed) & ((1 << 64) - 1)
    idx = _index(B, T)
    x = (idx & _M32).astype(np.uint32) ^ np.uint32(seed & 0xFFFFFFFF)

    def finalise(x):
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7FEB352D)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846CA68B)
        return x ^ (x >> np.uint32(16))

    x = finalise(x)
    x = x + ((idx >> np.uint64(32)).astype(np.uint32) * np.uint32(0x9E3779B9) + np.uint32(seed >> 32))
    x = finalise(x)
    return _unit(x >> np.uint32(8), B, T)


def unit_noise_ola(seed, B, T):
    """`noise_u` of csrc/spectral_ola.hip (the splitmix64 finaliser of seed + golden * (idx + 1)), top 24 bits / 2**24."""
    seed = np.uint64(int(seed) & ((1 << 64) - 1))
    z = seed + np.uint64(0x9E3779B97F4A7C15) * (_index(B, T) + np.uint64(1))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return _unit((z >> np.uint64(40)).astype(np.uint32), B, T)
