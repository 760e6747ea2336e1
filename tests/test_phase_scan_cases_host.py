"""CPU: the references of tests/phase_scan_cases.py satisfy, on their own, every condition tests/test_gpu_phase_scan.py puts on
the device - so a failure there is the kernel's.

* The kernel's upsampling form (`upsample_model`: w1 = fl32(scale * t) - t // hop) gives the bits of ATen's
  `frames_to_samples` at every case's hop, 48 and 100 included.  `oracle.dsp.frames_to_samples_closed_form` does so at the
  power-of-two hops; at 48 and 100 its weight fl32((t % hop) / hop) is another rounding of the same number than
  fl32(scale * t) - m (110 of 384 and 314 of 600 samples differ): scale and the product each round once at a magnitude up
  to Fr, 2 x 2^-24 x Fr in the weight, so there it is held to Fr x 2^-23 x the largest frame value, not to the bits.
* precise: the oracle's fp32 rot is within 2^-24 of rot64 (it is the same number rounded once: 2^-26).
* train mode: the kernel's summation order (`train_rot_model`) against the oracle's sequential sum: at most one fp32 ulp of the
  largest |S| apart, at most 1e-4 of the samples beyond 2^-24.  Measured: no sample differs in any case, the 1.3 M of the
  long case included (a flip needs an fp64 sum within ~1e-13 relative of an fp32 rounding boundary).
* comb: E32 is rounding-sized and `comb_model` is at most COMB_MODEL_RATIO x max(E32, 2^-23) from comb64; the ratio is in the
  assert message.  Measured over all cases, both modes, with and without init: E32 8.9e-8..1.8e-7, model 6.4e-8..1.7e-7,
  ratio 0.51..1.12 (the largest at B2-Fr4-hop48 precise with init)."""
import numpy as np
import pytest
import torch

import phase_scan_cases as C
from oracle import dsp as O

RUNS, RUN_IDS = C.runs()
CASE_INIT = sorted({(c, w) for c, _, w in RUNS}, key=lambda cw: (C.CASES.index(cw[0]), cw[1]))
CASE_INIT_IDS = ["%s-%s" % (C.case_id(c), "init" if w else "noinit") for c, w in CASE_INIT]


def test_case_table():
    assert len(C.CASES) == 13 and len(set(C.case_id(c) for c in C.CASES)) == 13
    assert len(RUNS) == 11 * 4 + 2 * 2
    for c in C.CASES:
        B, Fr, hop = c[:3]
        assert 1 <= hop <= 1024 and Fr * hop < 1 << 24
        assert (B * Fr * hop > 100_000) == (c == C.LONG_CASE)          # the long case is the only one above 100 k samples
    assert sum(1 for c in C.CASES if not c[5]) == 1 and C.CASES[10][2] == 512
    assert C.settings(C.LONG_CASE) == C.settings(C.HIGH_CASE) == ((True,), (1,))
    assert all(C.settings(c) == ((False, True), (0, 1, 2)) for c in C.FULL_CASES)
    assert {c[2] for c in C.CASES} == {1, 48, 100, 128, 256, 512, 1024}
    assert any(c[0] * c[1] % 4 for c in C.CASES if c[2] == 512) and any(c[0] * c[1] % 4 for c in C.CASES if c[2] != 512)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_tracks(case):
    B, Fr, hop, track = case[:4]
    f = C.f0_track(B, Fr, track, case[4])
    assert f.shape == (B, Fr, 1) and f.dtype == torch.float32
    assert torch.equal(f, C.f0_track(B, Fr, track, case[4]))
    k = C.case_ref(case, True)
    assert k["f0_up"].shape == k["rot64"].shape == (B, Fr * hop) and k["rot64"].dtype == torch.float64
    assert torch.equal(k["init"], torch.tensor(C.INIT)[torch.arange(B) % 3])
    if track == "voiced":
        assert 65 <= float(f.min()) and float(f.max()) <= 800
    elif track == "high":
        assert 1000 <= float(f.min()) and float(f.max()) <= 1600
    else:
        up = k["f0_up"]
        assert bool((up <= 0).any()) and bool((up > 0).any())         # the gate has both sides in every gaps case
        assert int((f == np.float32(0.05)).sum()) == 1
        if B >= 2:
            assert bool((up[1] == 0).all())                           # the all-zero row
        if Fr >= 3:
            assert float(f[0, 0]) == 0 and float(f[0, -1]) == 0
        if Fr >= 5:
            z = (f[0, 1:-1, 0] == 0).nonzero().flatten()
            assert len(z) >= 1 and bool((f[0, 1:-1, 0] > 0).any())      # a zero run inside, voiced frames around it
        # the bare 1e-3 denominator: arguments in the 1e7 range, past 2^24 where every fp32 is an even integer
        x = float(C.SR) * k["rot32"][True].double() / (up + 1e-3).double()
        assert float(x.abs().max()) > 2.0 ** 23


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_upsampling_forms(case):
    k = C.case_ref(case, False)
    hop = k["hop"]
    assert torch.equal(C.upsample_model(k["f0_frames"], hop), k["f0_up"])
    closed = O.frames_to_samples_closed_form(k["f0_frames"], hop).squeeze(-1)
    if hop & (hop - 1) == 0:
        assert torch.equal(closed, k["f0_up"])
    else:
        d = float((closed.double() - k["f0_up"].double()).abs().max())
        assert d <= k["Fr"] * 2.0 ** -23 * float(k["f0_frames"].abs().max()), (hop, d)


@pytest.mark.parametrize("case,with_init", CASE_INIT, ids=CASE_INIT_IDS)
def test_rot_references(case, with_init):
    k = C.case_ref(case, with_init)
    d = float(C.wrap_diff(k["rot32"][True], k["rot64"]).max())
    assert 0 < d <= C.ROT_TOL, d
    assert float(k["rot64"].abs().max()) <= 0.5
    model = C.train_rot_model(k["f0_up"], k["init"], k["hop"])
    assert model.dtype == torch.float32 and float(model.abs().max()) <= 0.5
    C.check_train_rot(f"{C.case_id(case)} summation-order model", model, k)
    if case == C.HIGH_CASE:
        # the purpose of the case: a coarser grid per sample than any voiced case of its length
        assert k["ulp_S"] >= 2.0 ** -14
    if case == C.LONG_CASE:
        assert k["ulp_S"] >= 2.0 ** -10


@pytest.mark.parametrize("case,precise,with_init", RUNS, ids=RUN_IDS)
def test_comb_model_against_reference_error(case, precise, with_init):
    k = C.case_ref(case, with_init)
    rot, f0 = k["rot32"][precise], k["f0_up"]
    c64, c32, cm = C.comb64(rot, f0), C.comb32(rot, f0), C.comb_model(rot, f0)
    assert c64.dtype == torch.float64 and c32.dtype == torch.float32 and cm.dtype == torch.float32
    assert bool(torch.isfinite(cm).all()) and bool(torch.isfinite(c64).all())
    e32 = float((c32.double() - c64).abs().max())
    em = float((cm.double() - c64).abs().max())
    ratio = em / max(e32, C.COMB_FLOOR)
    msg = f"{C.case_id(case)}: E32 {e32:.3e}, model {em:.3e} = {ratio:.2f} x max(E32, 2^-23)"
    print("COMB", msg)
    assert 2.0 ** -24 < e32 < 2.0 ** -21, msg          # rounding-sized: K_COMB x E32 stays below 1e-5
    assert ratio <= C.COMB_MODEL_RATIO, msg
    assert C.K_COMB == 16.0 * C.COMB_MODEL_RATIO
    # gating: the oracle's own mode 2 is mode 1 with exact zeros where f0 <= 0
    g32 = C.comb32(rot, f0, True)
    un = f0 <= 0
    assert bool((g32[un] == 0).all()) and torch.equal(g32[~un], c32[~un])
    if case[3] == "gaps" and not with_init and case[0] >= 2:
        assert bool((c64[1] == 1.0).all()) and bool((cm[1] == 1.0).all())   # zero row, no init: rot == 0, sinc(0) == 1
