"""Stage tests of `ddsp_phase_scan` (csrc/phase_scan.hip): both kernel pairs at every hop, gap and mode of
tests/phase_scan_cases.py, whose docstring lists the cases, the references and where each tolerance comes from
(tests/test_phase_scan_cases_host.py shows that the references alone meet them).  Nothing is masked out of a comparison.

Per (case, precise, init), over the case's comb modes:
  f0_up == the oracle's bits; phase == fl32(2 pi) * rot and phase_frames == phase[:, ::hop] bit for bit;
  precise: wrap-aware |rot - rot64| <= 2^-24;  train: <= one fp32 ulp of the largest |S| from the oracle's rot32 and at most
  1e-4 of the samples beyond 2^-24;
  comb against comb64 of the DEVICE's rot and f0_up: <= K_COMB x max(E32, 2^-23); mode 2 is exactly 0.0 where f0_up <= 0 and
  the bits of mode 1 elsewhere; mode 1 on the all-zero row without init is exactly 1.0;
  the comb mode changes no other output, and a second call gives the same bits.
Per case: every row alone equals its row of the batch; any subset of the optional outputs gives the same bits.
The unaligned case runs through views one float past a 16-byte boundary with sentinels around them.

MEASURED (MI355X), over all 48 runs (the PRECISE / TRAIN / COMB lines this file prints):
  precise |rot - rot64|      1.48e-8 .. 1.57e-8 (2^-26 = 1.49e-8 is the final rounding; the largest is the 2600-frame case)
                             against the bound 2^-24 = 5.96e-8
  train rot against rot32    no sample differs in any case, the 1.3 M of the long case included (bound: one ulp of |S|)
  comb against comb64        0.51 .. 1.12 x max(E32, 2^-23), at most 1.85e-7 absolute, against K_COMB = 20 x; run by run the
                             same ratios as the CPU restatement `comb_model` gives with the oracle's rot
  everything else            bit-equal as asserted
"""
import numpy as np
import pytest
import torch

from hipddsp import _ptr
import phase_scan_cases as C

pytestmark = pytest.mark.gpu

RUNS, RUN_IDS = C.runs()
OUTPUTS = ("rot", "phase", "comb", "f0_up", "phase_frames")
PAD, SENTINEL = 5, -777.0          # floats before (and 7 after) each unaligned view; 5 floats = 20 bytes: 4 past a 16-byte line


def _scan_views(ctx, dev, f0_frames, init, hop, precise, mode, want):
    """`ddsp_phase_scan` through the C entry with every requested output a view at 16 k + 4 bytes of a sentinel-filled
    buffer, so the dispatch takes the generic kernels at hop 512 too; the sentinels must survive."""
    B, Fr = f0_frames.shape[:2]
    f0 = f0_frames.reshape(B, Fr).contiguous().to(dev)
    ip = None if init is None else init.contiguous().to(dev)
    bufs, views = {}, {}
    for name in OUTPUTS:
        n = B * Fr if name == "phase_frames" else B * Fr * hop
        if name == "phase_frames" or (name == "comb" and mode != 0) or want.get(name, False):
            bufs[name] = torch.full((PAD + n + 7,), SENTINEL, device=dev, dtype=torch.float32)
            views[name] = bufs[name][PAD:PAD + n]
            assert views[name].data_ptr() % 16 == 4
        else:
            views[name] = None
    ctx.call("ddsp_phase_scan", _ptr(f0), _ptr(ip), B, Fr, int(hop), C.SR, 1 if precise else 0, int(mode),
             *(_ptr(views[n]) for n in OUTPUTS))
    out = {}
    for name in OUTPUTS:
        if views[name] is None:
            out[name] = None
            continue
        whole = bufs[name].cpu()
        n = views[name].numel()
        assert bool((whole[:PAD] == SENTINEL).all()) and bool((whole[PAD + n:] == SENTINEL).all()), f"{name}: wrote outside its view"
        out[name] = whole[PAD:PAD + n].reshape(B, -1).clone()
    return out


def _scan(ctx, dev, case, k, precise, mode, rows=None, rot=True, phase=True, f0=True):
    """One call -> {name: host tensor or None}; `rows` selects a slice of the batch."""
    f0_frames, init = k["f0_frames"], k["init"]
    if rows is not None:
        f0_frames = f0_frames[rows]
        init = None if init is None else init[rows]
    if not case[5]:
        return _scan_views(ctx, dev, f0_frames, init, k["hop"], precise, mode, {"rot": rot, "phase": phase, "f0_up": f0})
    out = ctx.phase_scan(f0_frames.to(dev), k["hop"], C.SR, None if init is None else init.to(dev), precise, mode,
                         want_rot=rot, want_phase=phase, want_f0=f0)
    return {n: None if t is None else t.cpu() for n, t in out.items()}


def _same(what, a, b, names=OUTPUTS):
    for n in names:
        if a[n] is not None and b[n] is not None:
            assert torch.equal(a[n], b[n]), f"{what}: {n} differs"


def _check_comb(what, comb, rot, f0_up):
    c64, c32 = C.comb64(rot, f0_up), C.comb32(rot, f0_up)
    assert comb.dtype == torch.float32 and bool(torch.isfinite(comb).all()), what
    e32 = float((c32.double() - c64).abs().max())
    e = float((comb.double() - c64).abs().max())
    bound = C.K_COMB * max(e32, C.COMB_FLOOR)
    print(f"COMB {what}: max|comb - comb64| {e:.3e} = {e / max(e32, C.COMB_FLOOR):.2f} x max(E32 {e32:.3e}, 2^-23); bound {bound:.3e}")
    assert e <= bound, (what, e, e32, bound)


@pytest.mark.parametrize("case,precise,with_init", RUNS, ids=RUN_IDS)
def test_phase_scan_case(ctx, dev, case, precise, with_init):
    what = RUN_IDS[RUNS.index((case, precise, with_init))]
    k = C.case_ref(case, with_init)
    B, T, hop = k["B"], k["T"], k["hop"]
    modes = C.settings(case)[1]
    outs = {m: _scan(ctx, dev, case, k, precise, m) for m in modes}
    o = outs[modes[0]]
    rot, f0_up = o["rot"], o["f0_up"]
    assert rot.shape == (B, T) and o["phase_frames"].shape == (B, k["Fr"])

    assert torch.equal(f0_up, k["f0_up"]), f"{what}: f0_up is not the oracle's bits"
    assert float(rot.abs().max()) <= 0.5
    if precise:
        d = float(C.wrap_diff(rot, k["rot64"]).max())
        print(f"PRECISE {what}: max wrap-aware |rot - rot64| {d:.3e} (bound 2^-24 = {C.ROT_TOL:.3e})")
        assert d <= C.ROT_TOL, (what, d)
    else:
        C.check_train_rot(what, rot, k)
    assert torch.equal(o["phase"], rot * torch.tensor(C.TWO_PI32, dtype=torch.float32)), f"{what}: phase != fl32(2 pi) * rot"
    assert torch.equal(o["phase_frames"], o["phase"][:, ::hop]), f"{what}: phase_frames != phase[:, ::hop]"

    for m in modes[1:]:
        _same(f"{what}: comb_mode {m} against {modes[0]}", outs[m], o, ("rot", "phase", "f0_up", "phase_frames"))
    if 0 in outs:
        assert outs[0]["comb"] is None
    if 1 in outs:
        comb = outs[1]["comb"]
        _check_comb(what, comb, rot, f0_up)
        if case[3] == "gaps" and B >= 2 and not with_init:
            assert bool((f0_up[1] == 0).all()) and bool((comb[1] == 1.0).all()), f"{what}: comb of the silent row is not 1.0"
    if 2 in outs:
        gated, un = outs[2]["comb"], f0_up <= 0
        assert bool((gated[un] == 0.0).all()), f"{what}: gated comb is not 0.0 at {int((gated[un] != 0).sum())} of {int(un.sum())} unvoiced samples"
        assert torch.equal(gated[~un], outs[1]["comb"][~un]), f"{what}: gated comb differs from mode 1 at voiced samples"
        if case[3] == "gaps":
            assert bool(un.any()) and bool((~un).any())
    _same(f"{what}: second call", _scan(ctx, dev, case, k, precise, modes[-1]), outs[modes[-1]])


@pytest.mark.parametrize("case", [c for c in C.CASES if c[0] >= 2], ids=C.case_id)
def test_rows_are_independent(ctx, dev, case):
    """A row run alone (B = 1) gives the bits of its row in the batch: the prefix stays inside its utterance."""
    k = C.case_ref(case, True)
    mode = C.settings(case)[1][-1]
    for precise in (True, False):
        batch = _scan(ctx, dev, case, k, precise, mode)
        for b in range(k["B"]):
            alone = _scan(ctx, dev, case, k, precise, mode, rows=slice(b, b + 1))
            _same(f"{C.case_id(case)} precise={precise} row {b}", alone, {n: batch[n][b:b + 1] for n in OUTPUTS})


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_optional_outputs(ctx, dev, case):
    """No optional output, or any single one, leaves the bits of what is written - and phase_frames - as they are."""
    k = C.case_ref(case, True)
    for precise in (True, False):
        full = _scan(ctx, dev, case, k, precise, 1)
        for name, kw, mode in (("none", {}, 0), ("rot", {"rot": True}, 0), ("phase", {"phase": True}, 0),
                               ("f0_up", {"f0": True}, 0), ("comb", {}, 1)):
            want = dict(rot=False, phase=False, f0=False)
            want.update(kw)
            part = _scan(ctx, dev, case, k, precise, mode, **want)
            written = {n for n in OUTPUTS if part[n] is not None}
            assert written == {"phase_frames"} | ({name} if name != "none" else set()), (name, written)
            _same(f"{C.case_id(case)} precise={precise} only {name}", part, full)
