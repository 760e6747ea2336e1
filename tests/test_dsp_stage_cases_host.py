"""CPU: the cases of tests/dsp_stage_cases.py are what tests/test_gpu_dsp_stages.py takes them for.

The device tests bound the device's error by 16 x E32, the float32 oracle's own distance from the float64 one.  That means
something only while E32 is a rounding-sized number: not zero (a float32 pass that silently ran in float64), not large (an
ill-conditioned case, where 16 x E32 would let a structural error through).  So: 1e-8 < E32 < 1e-5 for every forward output
and every gradient that the device tests compare, the subsets and blocks they compare separately included."""
import numpy as np
import pytest
import torch

import dsp_stage_cases as C

LO, HI = 1e-8, 1e-5


def _bank(c):
    B, Fr, H, hop, col0, seed = c
    return C.bank_case(B, Fr, H, hop, seed, col0)


def _ola(c):
    B, Fr, seed, comb = c
    return C.ola_case(B, Fr, seed, comb)


@pytest.mark.parametrize("case", C.BANK_CASES, ids=C.bank_id)
def test_bank_reference_error_is_rounding_sized(case):
    k = _bank(case)
    B, Fr, H, hop = case[:4]
    assert k["y64"].dtype == torch.float64 and k["y32"].dtype == torch.float32
    assert k["d64"].dtype == torch.float64 and k["d32"].dtype == torch.float32
    assert k["y64"].shape == (B, Fr * hop) and k["d64"].shape == (B, Fr, H)
    assert LO < C.rel_err(k["y32"], k["y64"]) < HI
    assert LO < C.rel_err(k["d32"], k["d64"]) < HI
    m = k["masked"]
    for sel in (m, ~m):
        if sel.any():
            assert LO < C.rel_err(k["d32"][sel], k["d64"][sel]) < HI
            assert C.max_err(k["d32"][sel], k["d64"][sel]) > 0


@pytest.mark.parametrize("case", C.BANK_CASES, ids=C.bank_id)
def test_bank_masks(case):
    k = _bank(case)
    H, m = case[2], k["masked"]
    if H >= 37:
        assert m.any() and (~m).any()
    assert float(k["f0_frames"][0, 0]) == 441.0
    if H >= 50:
        # 441 * 50 == 22050.0 == fmax exactly: `<` is strict
        assert np.float32(441.0) * np.float32(50.0) == np.float32(C.FMAX)
        assert bool(m[0, 0, 49]) and not bool(m[0, 0, 48])
    # masked harmonics keep 1e-7 of their amplitude: their gradient is small, not zero
    if m.any():
        assert float(k["d64"][m].abs().max()) > 0
        assert float(k["d64"][m].norm()) < 1e-5 * float(k["d64"][~m].norm())


@pytest.mark.parametrize("case", C.OLA_CASES, ids=C.ola_id)
def test_ola_reference_error_is_rounding_sized(case):
    k = _ola(case)
    B, Fr = case[:2]
    assert k["ctrl"].shape == (B * Fr, 3 * C.NB + 5)
    assert k["y64"].dtype == torch.float64 and k["y32"].dtype == torch.float32
    assert k["y64"].shape == (B, Fr * C.OLA_HOP) and k["d64"].shape == (B * Fr, 3 * C.NB)
    assert float(k["u"].min()) >= 0.0 and float(k["u"].max()) < 1.0
    assert LO < C.rel_err(k["y32"], k["y64"]) < HI
    assert LO < C.rel_err(k["d32"], k["d64"]) < HI
    for s in C.OLA_BLOCKS.values():
        assert LO < C.rel_err(k["d32"][:, s], k["d64"][:, s]) < HI


def test_lds_range_case_reference_error():
    """H = 2048 (tests/test_gpu_dsp_stages.py::test_sins_bank_bwd_lds_range).  The only frame is at 441 Hz: harmonics 1..49
    are unmasked and decide the output and the gradient as a whole, where 16 x E32 stays far under the project's 1e-4 gate.
    The masked ones reach k * phase = 2048 * pi, whose float32 rounding (half an ulp of up to 6434: 2.4e-4 rad) is the oracle's
    own error there and the kernel's as well (it seeds every block of 32 harmonics from the same rounded product): E32 of that
    subset is a few 1e-5, on entries that carry 1e-7 of the weight."""
    k = C.bank_case(*C.LDS_RANGE_CASE)
    m = k["masked"]
    assert int((~m).sum()) == 49
    for e in (C.rel_err(k["y32"], k["y64"]), C.rel_err(k["d32"], k["d64"]), C.rel_err(k["d32"][~m], k["d64"][~m])):
        assert LO < e < HI, e
    assert LO < C.rel_err(k["d32"][m], k["d64"][m]) < 1e-4


@pytest.mark.parametrize("gen", [C.unit_noise_fir, C.unit_noise_ola], ids=["fir", "ola"])
def test_generator_restatements(gen):
    B, T = 2, 1 << 15
    u = gen(5, B, T)
    assert u.shape == (B, T) and u.dtype == np.float32
    assert u.min() >= 0.0 and u.max() < 1.0
    grid = u.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(grid, np.floor(grid))                   # on the 24-bit grid
    assert abs(float(u.astype(np.float64).mean()) - 0.5) < 0.01     # over 2**16 samples
    assert not np.array_equal(u, gen(5 + 2 ** 32, B, T))          # the high seed word counts
    assert np.mean(u == gen(5 + 2 ** 32, B, T)) < 1e-3
    assert np.array_equal(u, gen(5, B, T))
    # the index is b * T + t: row 1 continues row 0
    assert np.array_equal(u.reshape(-1), gen(5, 1, B * T).reshape(-1))


def test_generators_differ_from_each_other():
    a, b = C.unit_noise_fir(5, 2, 4096), C.unit_noise_ola(5, 2, 4096)
    assert np.mean(a == b) < 1e-3
