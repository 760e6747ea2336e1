"""CPU: the fixtures of tests/golden/make_golden_hop.py are what tests/test_gpu_hop.py takes them for.

  - the case tables reach what they are there for (every Fr of {1, 2, 5, 9} and n of {32, 510, 1022, 2046} per hop, the filter
    longer than the signal, the smallest call, an add_in case per hop; OLA Fr of {1, 2, 5});
  - every case has its arrays, of the shapes and dtypes the inputs regenerated from the seeds imply, all finite;
  - the stored reference results belong to those inputs: the project's oracle (oracle/dsp.py takes the hop from its arguments)
    reproduces the FIR outputs to 1e-6 rms (the bound test_gpu_dsp.py:115 puts on the oracle's own two forms) and the OLA
    outputs to a few E32;
  - the OLA's E32 (the float32 reference against the float64 one), which scales the device's bound, is rounding-sized: between
    1e-8 and 1e-5 relative, as tests/test_dsp_stage_cases_host.py holds it at 512;
  - no fixture is near the size limit of a committed file."""
import os

import numpy as np
import pytest
import torch

import dsp_stage_cases as SC
import hop_cases as H
from conftest import GOLDEN, rms
from oracle import dsp as O

FILES = ("hop_fir_128.npz", "hop_fir_256.npz", "hop_ola.npz", "hop_models.npz")


@pytest.fixture(scope="module")
def fix():
    z = {}
    for name in FILES:
        with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as f:
            z.update({k: f[k] for k in f.files})
    return z


def test_case_tables_reach_their_rules():
    for hop in H.HOPS:
        mine = [c for c in H.FIR_CASES if c[0] == hop]
        assert {c[1] for c in mine} >= {1, 2, 5, 9} and {c[2] for c in mine} == {32, 510, 1022, 2046}
        assert any(c[1] == 1 and c[2] == 32 for c in mine) and any(c[3] for c in mine)
        assert hop == 256 or any(c[1] * hop % 256 for c in mine)  # hop 128: a partial last tile of 256 samples
        assert hop == 128 or any(c[1] * hop > 2048 for c in mine) # hop 256: more than one block of 2048 samples
        assert {c[1] for c in H.OLA_CASES if c[0] == hop} == {1, 2, 5}
    assert (128, 3, 2046, False) in H.FIR_CASES and 2046 > 3 * 128
    assert len(set(H.FIR_CASES)) == len(H.FIR_CASES)
    assert max(H.LOSS_SCALES) < H.MODEL_FR * min(H.HOPS) and H.LOSS_RANGE[0] <= min(H.LOSS_SCALES)
    assert max(H.MODEL_RAGGED) == H.MODEL_FR and min(H.MODEL_RAGGED) < H.MODEL_FR


def test_fixture_files_are_small():
    for name in FILES:
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 512 * 1024, name


@pytest.mark.parametrize("case", H.FIR_CASES, ids=H.fir_id)
def test_fir_fixture(fix, case):
    hop, Fr, n, _ = case
    x, ir, g, add = H.fir_inputs(case)
    assert x.shape == g.shape == add.shape == (H.B, Fr * hop) and ir.shape == (H.B, Fr, n)
    assert not torch.equal(x[0], x[1]) and not torch.equal(ir[0], ir[1])          # different rows
    y, dx, dir_ = (torch.from_numpy(fix[H.fir_key(case, k)]) for k in ("y", "dx", "dir"))
    assert y.dtype == dx.dtype == dir_.dtype == torch.float32
    assert y.shape == x.shape and dx.shape == x.shape and dir_.shape == ir.shape
    assert all(bool(torch.isfinite(v).all()) for v in (y, dx, dir_))
    assert 0.1 < rms(y) < 3.0                                                     # the scale of test_ltv_fir_small_vs_direct
    assert rms(y.double() - O.ltv_fir_fft(x.double(), ir.double())) < 1e-6
    xg = x.clone().requires_grad_(True)
    ig = ir.clone().requires_grad_(True)
    (O.ltv_fir_fft(xg, ig) * g).sum().backward()
    assert float((dx - xg.grad).norm() / xg.grad.norm()) < 2e-6 and float((dir_ - ig.grad).norm() / ig.grad.norm()) < 2e-6


@pytest.mark.parametrize("case", H.OLA_CASES, ids=H.ola_id)
def test_ola_fixture(fix, case):
    hop, Fr = case
    nb = hop + 1
    ctrl, comb, u, g = H.ola_inputs(case)
    assert ctrl.shape == (H.B * Fr, 3 * nb + H.OLA_PAD) and comb.shape == u.shape == g.shape == (H.B, Fr * hop)
    y32, y64, d32, d64 = (torch.from_numpy(fix[H.ola_key(case, k)]) for k in ("y32", "y64", "d32", "d64"))
    assert y32.dtype == d32.dtype == torch.float32 and y64.dtype == d64.dtype == torch.float64
    assert y32.shape == y64.shape == comb.shape and d32.shape == d64.shape == (H.B * Fr, 3 * nb)
    for a, b in ((y32, y64), (d32, d64)):
        e = SC.rel_err(a, b)
        print(f"MEASURED {H.ola_id(case)} E32 {e:.2e}")
        assert 1e-8 < e < 1e-5
    # the oracle's statement of the stage, at this hop, in float64, on the same inputs
    c = ctrl[:, :3 * nb].double()
    hm, hp, nm = (c[:, i * nb:(i + 1) * nb].reshape(H.B, Fr, nb) for i in range(3))
    want = O.windowed_spectral_ola(comb.double(), (2 * u - 1).double(), torch.exp(hm + 1j * np.pi * hp), torch.exp(nm) / 128, hop)
    assert SC.rel_err(y64, want) < 1e-12


@pytest.mark.parametrize("hop", H.HOPS)
@pytest.mark.parametrize("name", H.MODELS)
def test_model_fixture(fix, name, hop):
    T = H.MODEL_FR * hop
    parts = ("signal",) if name == "CombSubFast" else ("signal", "harmonic", "noise")
    for tag in ("infer", "train"):
        for part in parts:
            v = fix[H.model_key(name, hop, f"{part}_{tag}")]
            assert v.shape == (H.B, T) and v.dtype == np.float32 and np.isfinite(v).all()
        assert rms(torch.from_numpy(fix[H.model_key(name, hop, "signal_" + tag)])) > 1e-3
    names, gn = fix[H.model_key(name, hop, "param_names")], fix[H.model_key(name, hop, "gradnorm")]
    assert len(names) == len(gn) > 10 and np.isfinite(gn).all() and (gn > 1e-6).sum() > len(gn) // 2
    assert np.isfinite(fix[H.model_key(name, hop, "loss")]) and float(fix[H.model_key(name, hop, "loss")]) > 0
