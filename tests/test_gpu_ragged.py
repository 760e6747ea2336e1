"""Ragged batches on the device: `forward(..., n_frames=)` renders rows of different length in one padded batch, each row as
if it had been rendered alone at its own length.

The yardstick is the CPU oracle (`oracle.synth.*_forward`, `oracle.ctrlnet.unit2control`) run ON EACH ROW ALONE AT ITS OWN
LENGTH - never another call of the library.  Gates are those of tests/test_gpu_models.py: waveforms rms < 1e-4 (BASELINE north
star), control matrix rms < 2e-5 and max < 2e-4, frame phases to 1e-6 of a turn.  After the inputs are made, all padding of
units / f0 / volume / noise is overwritten, once with large finite garbage and once with NaN."""
import os

import numpy as np
import pytest
import torch

import synthetic
from conftest import GOLDEN, rms
from oracle import ctrlnet as OC
from oracle import realtime as ORT
from oracle import synth as OS

pytestmark = pytest.mark.gpu
HOP = 512
GATE = 1e-4


def poison(inp, lengths, kind, hop=HOP):
    """A copy of the inputs whose padding (frames >= lengths[b], samples >= lengths[b] * hop) holds garbage or NaN."""
    d = {k: v.clone() for k, v in inp.items()}
    nan = float("nan")
    for b, n in enumerate(lengths):
        pad = d["units"].shape[1] - n
        if pad == 0:
            continue
        if kind == "nan":
            d["units"][b, n:] = nan
            d["f0"][b, n:] = nan
            d["volume"][b, n:] = nan
        else:
            sign = torch.tensor([1.0, -1.0]).repeat((pad * d["units"].shape[2] + 1) // 2)[:pad * d["units"].shape[2]]
            d["units"][b, n:] = 1e4 * sign.reshape(pad, -1)
            d["f0"][b, n:, 0] = torch.tensor([-1.0, 0.0, 1e5]).repeat(pad // 3 + 1)[:pad]
            d["volume"][b, n:] = 1e3
        if "noise" in d:
            d["noise"][b, n * hop:] = nan if kind == "nan" else 1e4
    return d


def _to(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def _causal_model(name, seed):
    from ddsp.vocoder import CombSub
    ref_model, cfg = synthetic.build_model(name, seed=seed)
    model = CombSub(44100, 512, cfg["n_mag_allpass"], cfg["n_mag_harmonic"], cfg["n_mag_noise"], 256, cfg["n_spk"], c=True)
    model.load_state_dict(ref_model.state_dict(), strict=True)
    return model.eval(), dict(cfg, c=True)


def _big_lengths():
    rng = np.random.Generator(np.random.PCG64(48172))
    n = [int(x) for x in rng.integers(20, 173, size=48)]
    n[17] = 172
    return n


def _mid_lengths():
    rng = np.random.Generator(np.random.PCG64(20100))
    n = [int(x) for x in rng.integers(1, 101, size=20)]
    n[3], n[11] = 100, 17
    return n


# total padded rows <= 256: the K-split launches whose partial sums ride in the next GroupNorm / LayerNorm pass; just above:
# whole-K launches; >= 8192: pre-split activations, the LayerNorms fused into the GEMMs, the split-bf16 attention kernel;
# "kv_whole" (beyond the issue's list): 20 rows x 8 heads = 160 (utterance, head) pairs > 128 and 2000 rows < 8192 - the fp32
# attention with one wave per feature tile walking all frame tiles (performer_kv_kernel), which the other three do not reach
REGIMES = {"ksplit": [80, 12, 1], "whole_k": [172, 87, 33, 3], "fused": _big_lengths(), "kv_whole": _mid_lengths()}


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("spk_mode", ["per_row", "broadcast", "mix"])
@pytest.mark.parametrize("regime", list(REGIMES))
def test_unit2ctrl_ragged_matches_oracle_rows(dev, lib_path, regime, spk_mode, causal):
    lengths = REGIMES[regime]
    B, Fr = len(lengths), max(lengths)
    if causal:
        model, cfg = _causal_model("CombSub", 99)
    else:
        model, cfg = synthetic.build_model("CombSub", seed=99)
    sd = {k[len("unit2ctrl."):]: v for k, v in model.state_dict().items() if k.startswith("unit2ctrl.")}
    inp = synthetic.make_inputs(4321 + B, B, Fr, with_noise=False)
    inp["phase"] = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).uniform(-np.pi, np.pi, (B, Fr)).astype(np.float32))
    spk = inp.pop("spk_id")
    spk = spk if spk_mode == "per_row" else spk[:1]
    mix = {3: 0.5, 10: 0.2, 99: 0.3} if spk_mode == "mix" else None
    want = []
    with torch.no_grad():
        for b, n in enumerate(lengths):
            want.append(OC.unit2control(sd, inp["units"][b:b + 1, :n], inp["f0"][b:b + 1, :n], inp["phase"][b:b + 1, :n],
                                        inp["volume"][b:b + 1, :n], spk[b:b + 1] if spk_mode == "per_row" else spk, mix,
                                        model.unit2ctrl.output_splits, return_flat=True, causal=causal)[0])
    model = model.to(dev)
    for kind in ("garbage", "nan"):
        d = poison(inp, lengths, kind)
        d["phase"] = inp["phase"].clone()
        for b, n in enumerate(lengths):
            d["phase"][b, n:] = float("nan") if kind == "nan" else 1e3
        d = _to(d, dev)
        with torch.no_grad():
            got = model.unit2ctrl.forward_flat(d["units"], d["f0"], d["phase"], d["volume"], spk.to(dev), mix,
                                               n_frames=lengths).cpu()
        assert got.shape == (B, Fr, model.unit2ctrl.n_out)
        errs = [((got[b, :n] - want[b]).abs().max().item(), rms(got[b, :n] - want[b])) for b, n in enumerate(lengths)]
        print(regime, spk_mode, causal, kind, "max", max(e[0] for e in errs), "rms", max(e[1] for e in errs))
        for b, (emax, erms) in enumerate(errs):
            assert emax < 2e-4 and erms < 2e-5, (kind, b, lengths[b], emax, erms)


def _oracle_rows(name, sd, cfg, inp, lengths, infer, ip, hop=HOP):
    rows = []
    with torch.no_grad():
        for b, n in enumerate(lengths):
            sig, ph, (hm, nz), _ = OS.FORWARD[name](sd, cfg, inp["units"][b:b + 1, :n], inp["f0"][b:b + 1, :n],
                                                    inp["volume"][b:b + 1, :n], inp["spk_id"][b:b + 1],
                                                    initial_phase=None if ip is None else ip[b:b + 1], infer=infer,
                                                    noise=inp["noise"][b:b + 1, :n * hop])
            rows.append(dict(signal=sig[0], phase=ph[0, :, 0], harmonic=hm[0], noise=nz[0]))
    return rows


def _check_rows(name, out, rows, lengths, tag, hop=HOP):
    sig, ph, (hm, nz) = out
    got = dict(signal=sig.cpu(), phase=ph.cpu()[:, :, 0], harmonic=hm.cpu(), noise=nz.cpu())
    for b, n in enumerate(lengths):
        T = n * hop
        pn = T if name == "Sins" else n                  # Sins returns the sample-rate phase
        for key in ("signal", "harmonic", "noise"):
            e = rms(got[key][b, :T] - rows[b][key])
            print(name, tag, "row", b, "frames", n, key, "rms", e)
            assert e < GATE, (name, tag, b, n, key, e)
            assert torch.count_nonzero(got[key][b, T:]) == 0 and torch.isfinite(got[key][b]).all(), (name, tag, b, key)
        dp = (got["phase"][b, :pn] - rows[b]["phase"]) / (2 * np.pi)
        assert (dp - torch.round(dp)).abs().max() < 1e-6, (name, tag, b, float((dp - torch.round(dp)).abs().max()))
        assert torch.count_nonzero(got["phase"][b, pn:]) == 0, (name, tag, b)


@pytest.mark.parametrize("infer", [True, False])
@pytest.mark.parametrize("name", ["CombSub", "Sins", "CombSubFast"])
def test_models_ragged_match_oracle_rows(dev, lib_path, name, infer):
    lengths = [1, 3, 20, 19, 11]
    B, Fr = len(lengths), max(lengths)
    model, cfg = synthetic.build_model(name, seed=7)
    sd = model.state_dict()
    inp = synthetic.make_inputs(2025 + Fr, B, Fr)
    ip = torch.tensor([1.0, -2.0, 0.5, 3.0, -0.25])
    rows = _oracle_rows(name, sd, cfg, inp, lengths, infer, ip)
    model = model.to(dev)
    for kind in ("garbage", "nan"):
        d = _to(poison(inp, lengths, kind), dev)
        with torch.no_grad():
            out = model(d["units"], d["f0"], d["volume"], d["spk_id"], initial_phase=ip.to(dev), infer=infer, noise=d["noise"],
                        n_frames=lengths)
        assert out[0].shape == (B, Fr * HOP)
        _check_rows(name, out, rows, lengths, f"infer={infer} {kind}")
    # in-kernel noise: repeatable for a seed, finite, zero past the rows, and the harmonic part is the injected-noise call's
    with torch.no_grad():
        a = model(d["units"], d["f0"], d["volume"], d["spk_id"], initial_phase=ip.to(dev), infer=infer, noise_seed=11,
                  n_frames=lengths)
        b_ = model(d["units"], d["f0"], d["volume"], d["spk_id"], initial_phase=ip.to(dev), infer=infer, noise_seed=11,
                   n_frames=torch.tensor(lengths))
    assert torch.equal(a[0], b_[0]) and torch.isfinite(a[0]).all()
    if name != "CombSubFast":
        assert torch.equal(a[2][0], out[2][0])
        assert 0.5 < rms(a[2][1][2, :20 * HOP]) / rms(out[2][1][2, :20 * HOP]) < 2.0
    for b, n in enumerate(lengths):
        assert torch.count_nonzero(a[0][b, n * HOP:]) == 0


@pytest.mark.parametrize("name", ["CombSub", "CombSubFast"])
def test_a_row_does_not_move_with_its_neighbours(dev, lib_path, name):
    """The same utterance (33 frames) in two different batches: both results meet the oracle gate of the row alone."""
    model, cfg = synthetic.build_model(name, seed=7)
    sd = model.state_dict()
    row = synthetic.make_inputs(77, 1, 33)
    want = _oracle_rows(name, sd, cfg, row, [33], True, None)[0]
    model = model.to(dev)
    for seed, lengths, at in ((1, [60, 33, 5], 1), (2, [33, 90, 90, 12, 1, 47], 0)):
        B, Fr = len(lengths), max(lengths)
        inp = synthetic.make_inputs(seed, B, Fr)
        for k in ("units", "f0", "volume"):
            inp[k][at, :33] = row[k][0]
        inp["noise"][at, :33 * HOP] = row["noise"][0]
        inp["spk_id"][at] = row["spk_id"][0]
        d = _to(poison(inp, lengths, "garbage"), dev)
        with torch.no_grad():
            sig = model(d["units"], d["f0"], d["volume"], d["spk_id"], noise=d["noise"], n_frames=lengths)[0]
        e = rms(sig[at, :33 * HOP].cpu() - want["signal"])
        print(name, "batch", lengths, "rms", e)
        assert e < GATE, (lengths, e)


def test_rectangular_call_is_untouched_and_full_counts_meet_the_gate(dev, lib_path):
    """n_frames=None: the launches of the parent commit (the row-kernel family is counted as
    test_unit2ctrl_large_batch_fused_glu_matches_oracle counts it) and, with them, its bits; n_frames=[Fr]*B: the ragged
    path on full rows meets the oracle gate of the rectangular batch."""
    import hipddsp
    model, cfg = synthetic.build_model("CombSub", seed=7)
    sd = model.state_dict()
    B, Fr = 2, 24
    inp = synthetic.make_inputs(31, B, Fr)
    with torch.no_grad():
        want = OS.combsub_forward(sd, cfg, inp["units"], inp["f0"], inp["volume"], inp["spk_id"], noise=inp["noise"])
    model = model.to(dev)
    d = _to(inp, dev)
    ctx = hipddsp.context_for(dev)

    def run(**kw):
        ctx.profile_begin(["u2c_rowwise", "other"])
        with torch.no_grad():
            out = model(d["units"], d["f0"], d["volume"], d["spk_id"], noise=d["noise"], **kw)
        prof = ctx.profile_end()
        return out, prof["u2c_rowwise"]["launches"], prof.get("other", {"launches": 0})["launches"]

    rect, rows_rect, other_rect = run()
    again, _, _ = run(n_frames=None)
    full, rows_full, other_full = run(n_frames=[Fr] * B)
    assert rows_rect == 12, rows_rect                                        # GroupNorm 2, LayerNorm 7, depthwise 3
    assert rows_full == rows_rect and other_full > other_rect                # the ragged helpers are launches of their own
    assert torch.equal(rect[0], again[0]) and torch.equal(rect[2][0], again[2][0])
    for got, tag in ((rect, "rect"), (full, "full")):
        assert rms(got[0].cpu() - want[0]) < GATE and rms(got[2][0].cpu() - want[2][0]) < GATE, tag
        assert rms(got[2][1].cpu() - want[2][1]) < GATE, tag


def test_ragged_against_reference_fixture(dev, lib_path):
    """tests/golden/ragged_models.npz: the REFERENCE's own forwards on rows of 12, 5, 1 and 9 frames, each alone
    (tests/golden/make_golden_ragged.py); here the four rows are one ragged call."""
    z = np.load(os.path.join(GOLDEN, "ragged_models.npz"), allow_pickle=False)
    lengths = [int(n) for n in z["lengths"]]
    assert lengths == [12, 5, 1, 9]
    inp = synthetic.make_inputs(int(z["seed_inputs"]), len(lengths), max(lengths))
    for name in ("CombSub", "Sins", "CombSubFast"):
        model, cfg = synthetic.build_model(name, seed=int(z["seed_weights"]), device=dev)
        for kind in ("garbage", "nan"):
            d = _to(poison(inp, lengths, kind), dev)
            with torch.no_grad():
                sig, ph, (hm, nz) = model(d["units"], d["f0"], d["volume"], d["spk_id"], noise=d["noise"], n_frames=lengths)
            for b, n in enumerate(lengths):
                T = n * HOP
                keys = [("signal", sig)] + ([("harmonic", hm), ("noise", nz)] if name != "CombSubFast" else [])
                for key, got in keys:
                    e = rms(got[b, :T].cpu() - torch.from_numpy(z[f"{name}_{key}_{b}"]))
                    print(name, kind, "row", b, key, "rms", e)
                    assert e < GATE, (name, kind, b, key, e)
                    assert torch.count_nonzero(got[b, T:]) == 0
                pf = ph[b, :T:HOP, 0] if name == "Sins" else ph[b, :n, 0]
                dp = (pf.cpu() - torch.from_numpy(z[f"{name}_phase_{b}"])) / (2 * np.pi)
                assert (dp - torch.round(dp)).abs().max() < 1e-6, (name, kind, b)


@pytest.mark.parametrize("name", ["CombSub", "CombSubFast"])
def test_render_in_ragged_batches_against_a_host_stitch_of_oracle_rows(dev, lib_path, name):
    """`infer_offline.render(batch_frames=)` on five slices with gaps, one abutting and one overlapping pair (the silence
    and the cross-fade branch), injected per-slice noise, against per-slice oracle outputs gated with the whole file's
    volume gate and joined by the rule of main.py:165-174 on the host."""
    import infer_offline
    from ddsp.vocoder import DotDict
    lens, starts = [40, 173, 9, 260, 88], [0, 45, 218, 225, 500]
    Fr = 600
    model, cfg = synthetic.build_model(name, seed=7)
    sd = model.state_dict()
    whole = synthetic.make_inputs(909, 1, Fr, with_noise=False)
    whole["volume"][0, 100:130] = 0.0                    # a gated stretch inside slice 1
    whole["volume"][0, 520:524] = 0.0
    rng = np.random.Generator(np.random.PCG64(910))
    units = [torch.from_numpy(rng.standard_normal((1, n, 256), dtype=np.float32)) for n in lens]
    noise = [torch.from_numpy(rng.random(n * HOP, dtype=np.float32)) for n in lens]
    spk = whole["spk_id"]
    gate = ORT.volume_gate(whole["volume"][0].numpy(), -60, HOP)
    result, current = np.zeros(0), 0
    with torch.no_grad():
        for s, n, u, nz in zip(starts, lens, units, noise):
            sig = OS.FORWARD[name](sd, cfg, u, whole["f0"][:, s:s + n], whole["volume"][:, s:s + n], spk, noise=nz[None])[0]
            out = (sig * gate[:, s * HOP:(s + n) * HOP]).squeeze().numpy()
            silent = s * HOP - current
            if silent >= 0:
                result = np.append(np.append(result, np.zeros(silent)), out)
            else:
                result = ORT.slice_cross_fade(result, out, current + silent)
            current = current + silent + len(out)
    model = model.to(dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": synthetic.SR}})
    segments = [(s, u.to(dev)) for s, u in zip(starts, units)]
    for batch_frames in (400, 1000, 1):
        got, sr = infer_offline.render(model, args, segments, whole["f0"].to(dev), whole["volume"].to(dev), spk.to(dev),
                                       noise=[z.to(dev) for z in noise], batch_frames=batch_frames)
        assert sr == synthetic.SR and got.shape == result.shape
        e = float(np.sqrt(np.mean((got - result) ** 2)))
        print(name, "batch_frames", batch_frames, "rms", e)
        assert e < GATE, (batch_frames, e)
    # noise_seed keeps meaning "repeatable"
    a = infer_offline.render(model, args, segments, whole["f0"].to(dev), whole["volume"].to(dev), spk.to(dev), noise_seed=3,
                             batch_frames=400)[0]
    b = infer_offline.render(model, args, segments, whole["f0"].to(dev), whole["volume"].to(dev), spk.to(dev), noise_seed=3,
                             batch_frames=400)[0]
    assert np.array_equal(a, b) and np.isfinite(a).all()


def test_ragged_refusals_on_the_device(dev, lib_path):
    model, cfg = synthetic.build_model("CombSub", seed=7, device=dev)
    d = _to(synthetic.make_inputs(5, 3, 8), dev)
    args = (d["units"], d["f0"], d["volume"], d["spk_id"])
    with pytest.raises(NotImplementedError, match="inference only"):
        model(*args, n_frames=[8, 3, 1])
    with pytest.raises(NotImplementedError, match="inference only"):
        model.unit2ctrl.forward_flat(d["units"], d["f0"], d["volume"], d["volume"], d["spk_id"], n_frames=[8, 3, 1])
    with torch.no_grad():
        for bad in ([8, 3], [8, 3, 0], [8, 3, 9], [8.0, 3, 1], torch.tensor([8, 3, 1], device=dev), torch.tensor([8.0, 3.0, 1.0])):
            with pytest.raises(ValueError):
                model(*args, n_frames=bad)
        for p in model.parameters():
            p.requires_grad_(False)
    sig = model(*args, n_frames=[8, 3, 1])[0]            # grad mode on, nothing wants a gradient: allowed
    assert torch.count_nonzero(sig[2, HOP:]) == 0
