"""The formant shift on the device: `ddsp_ctrl_warp` against its numpy statement (tests/formant_cases.py) bit for bit,
`forward_formant` of the three synthesisers against the eager composition, offline jobs with a formant, and
`StreamBank(formant=True)`.

Exactness.  The kernel owes the statement's bits in every element: both round once per operation and select at t == 0.
`forward_formant` against the composition (the model's own control-network call, the statement on the host, the model's
`_render`) runs the same kernels on the same bits: `torch.equal`, as tests/test_gpu_bank_glide.py holds its eager comparison.
Ragged, the composition ends as `_forward` does: the statement leaves the frames past a row's count alone, then every row's
last frame is held over its padding - the form `_render` takes a ragged batch in.  A job against the per-slice eager render is
held to rms < `GATE` = 1e-4, the method and the gate of tests/test_gpu_key_timeline.py's jobs-against-eager comparison (a ragged
group against slices rendered alone is not the same launch sequence)."""
import numpy as np
import pytest
import torch

import formant_cases as FC
import key_timeline_cases as KC
import synthetic
from conftest import rms
from test_bank_models_host import bank_model
from test_gpu_many import GATE
from test_gpu_many import encoder  # noqa: F401  (the module-scoped random-weight HubertSoft fixture)
from test_gpu_many_jobs import _args, _files, extractor  # noqa: F401

pytestmark = pytest.mark.gpu
SR, HOP = synthetic.SR, synthetic.HOP


def _i32(dev, a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev)


def _f32(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------------
JUST_BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))
FACTORS = [float(FC.factor(24)), float(FC.factor(-24)), float(FC.factor(1)), 1.0, JUST_BELOW_ONE]
# (rows, Fr, row stride, segments): 1539 = CombSubFast's row (not 16-byte aligned); 14 and 16: short rows, aligned and not
SHAPES = [(3, 3, 1539, [(0, 513, 0), (1026, 513, 0)]), (130, 1, 1539, [(0, 513, 0), (1026, 513, 0), (600, 1, 0)]),
          (130, 5, 14, [(0, 5, 1), (7, 2, 0)]), (3, 3, 16, [(0, 5, 1), (7, 2, 0), (12, 1, 1)]),
          (130, 13, 16, [(7, 2, 0), (0, 5, 1)])]


def _matrix(rows, width, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((rows, width)).astype(np.float32)
    specials = np.array([-0.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    at = rng.integers(0, rows * width, size=max(4, rows * width // 50))
    x.reshape(-1)[at] = specials[np.arange(at.size) % 4]
    return x


def _run(ctx, dev, x, segs, factors, Fr, **kw):
    got = _f32(dev, x)
    assert ctx.ctrl_warp_(got, segs, factors, Fr, **kw) is got
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("rows,Fr,width,segs", SHAPES)
def test_kernel_matches_the_statement(ctx, dev, lib_path, rows, Fr, width, segs):
    x, B = _matrix(rows, width, 31 + rows + width), rows // Fr
    rng = np.random.Generator(np.random.PCG64(5))
    ctx.poll_error()
    # a factor per frame: the five factors in turn
    per_frame = np.array([FACTORS[r % 5] for r in range(rows)], dtype=np.float32)
    want, err = FC.warp_rows(x, segs, per_frame, Fr)
    got = _run(ctx, dev, x, segs, _f32(dev, per_frame), Fr)
    assert not err and FC.same_bits(got, want) and not FC.same_bits(got, x)
    if Fr > 1:
        assert FC.same_bits(_run(ctx, dev, x, segs, _f32(dev, per_frame.reshape(B, Fr)), Fr), want)
    # a factor per batch row, with counts: the frames past a count keep their bits whatever the factor
    per_row = np.array([FACTORS[(b + 2) % 5] for b in range(B)], dtype=np.float32)
    counts = rng.integers(1, Fr + 1, size=B)
    want, _ = FC.warp_rows(x, segs, per_row, Fr, n_frames=counts)
    got = _run(ctx, dev, x, segs, _f32(dev, per_row), Fr, n_dev=_i32(dev, counts))
    assert FC.same_bits(got, want)
    for b in range(B):
        assert FC.same_bits(got[b * Fr + counts[b]:(b + 1) * Fr], x[b * Fr + counts[b]:(b + 1) * Fr])
    # the ragged form with a factor per frame whose padding holds garbage (NaN: no error word either)
    if Fr > 1:
        ragged = per_frame.reshape(B, Fr).copy()
        for b in range(B):
            ragged[b, counts[b]:] = np.nan
        want, _ = FC.warp_rows(x, segs, ragged, Fr, n_frames=counts)
        assert FC.same_bits(_run(ctx, dev, x, segs, _f32(dev, ragged), Fr, n_dev=_i32(dev, counts)), want)
    # through a row table with a -1 and an out-of-range entry: those rows keep their bits
    slots = np.array([(3 * b + 1) % 5 for b in range(B)], dtype=np.int32)
    slots[0], slots[B - 1] = -1, 5
    table = np.array([FACTORS[4], FACTORS[0], FACTORS[2], FACTORS[1], FACTORS[3]], dtype=np.float32)
    want, _ = FC.warp_rows(x, segs, table, Fr, slot_of_row=slots)
    got = _run(ctx, dev, x, segs, _f32(dev, table), Fr, slot_of_row=_i32(dev, slots))
    assert FC.same_bits(got, want) and FC.same_bits(got[:Fr], x[:Fr]) and FC.same_bits(got[-Fr:], x[-Fr:])
    # exactly 1 everywhere: the input's bits, -0.0, inf and NaN by selection
    assert FC.same_bits(_run(ctx, dev, x, segs, torch.ones(B, device=dev), Fr), x)
    ctx.poll_error()                                                                      # none of this raised the error word


def test_a_bad_factor_leaves_the_row_and_sets_the_error_word(ctx, dev, lib_path):
    """An error path that returns: no address depends on the factor."""
    rows, Fr, width, segs = 6, 3, 1539, [(0, 513, 0), (1026, 513, 0)]
    x = _matrix(rows, width, 77)
    for bad in (0.0, float("nan"), -1.0, float("inf")):
        torch.cuda.synchronize()
        ctx.poll_error()
        factors = np.array([bad, FACTORS[2]], dtype=np.float32)
        got = _run(ctx, dev, x, segs, _f32(dev, factors), Fr)
        want, err = FC.warp_rows(x, segs, factors, Fr)
        assert err and FC.same_bits(got, want) and FC.same_bits(got[:Fr], x[:Fr]) and not FC.same_bits(got[Fr:], x[Fr:])
        with pytest.raises(ValueError, match="ddsp_ctrl_warp"):
            ctx.poll_error()
        ctx.poll_error()                                                                  # read and cleared: reported once
        good = np.array([FACTORS[0], FACTORS[2]], dtype=np.float32)
        assert FC.same_bits(_run(ctx, dev, x, segs, _f32(dev, good), Fr), FC.warp_rows(x, segs, good, Fr)[0])
        ctx.poll_error()                                                                  # the next call is clean


# ---- 2. the models --------------------------------------------------------------------------------------------------------------
B, FR = 2, 9


@pytest.fixture(scope="module", params=["CombSub", "Sins", "CombSubFast"])
def model(request, dev, lib_path):
    return bank_model(request.param, 3, 43, dev)


def _inputs(dev, seed=6):
    z = synthetic.make_inputs(seed, B, FR, n_spk=3)
    return {k: v.to(dev) for k, v in z.items()}


def _outs(result):
    sig, phase, (harm, noise) = result
    return [sig, phase, harm, noise]


def _composition(model, d, factors, counts):
    """The eager composition: the control matrix of the model's own control-network call, the statement on the host, [ragged:
    every row's last frame over its padding,] the model's `_render`."""
    import hipddsp
    ctx = hipddsp.context_for(d["f0"].device)
    dev = d["f0"].device
    if counts is None:
        n_dev, f0 = None, d["f0"]
        ps = model._scan(ctx, f0, None, True)
        ctrl = model.unit2ctrl.forward_flat(d["units"], f0, ps["phase_frames"], d["volume"], d["spk_id"])
        excitation = lambda: model._noise_args(d["noise"], None)  # noqa: E731
    else:
        n_dev, units, f0, _, volume = model.unit2ctrl.hold_ragged(ctx, counts, d["units"], d["f0"], None, d["volume"])
        f0 = f0.reshape(B, FR, 1)
        ps = model._scan(ctx, f0, None, True)
        ctrl = model.unit2ctrl.forward_ragged(ctx, units, f0, ps["phase_frames"], volume, d["spk_id"], None, n_dev)
        excitation = lambda: model._ragged_noise(ctx, n_dev, B, FR, d["noise"], None)  # noqa: E731
    host = ctrl.reshape(B * FR, -1).cpu().numpy()
    warped, err = FC.warp_rows(host, model._formant_segments(), factors.cpu().numpy(), FR, n_frames=counts)
    assert not err and not FC.same_bits(warped, host)
    warped = warped.reshape(B, FR, -1)
    if counts is not None:
        for b, n in enumerate(counts):
            warped[b, n:] = warped[b, n - 1]
    outs, _ = model._render(ctx, torch.from_numpy(warped).to(dev), ps, f0, excitation, n_dev)
    return [outs[0], model._phase_out(ctx, ps, n_dev).unsqueeze(-1)] + list(outs[1:])


def test_zero_and_ones_are_forward(model, dev):
    d = _inputs(dev)
    with torch.no_grad():
        want = _outs(model(d["units"], d["f0"], d["volume"], d["spk_id"], noise=d["noise"]))
        for formant in (0, 0.0, torch.ones(B, device=dev), torch.ones(B, FR, device=dev)):
            got = _outs(model.forward_formant(d["units"], d["f0"], d["volume"], d["spk_id"], formant, noise=d["noise"]))
            assert all(torch.equal(a, b) for a, b in zip(got, want))
        ragged = _outs(model(d["units"], d["f0"], d["volume"], d["spk_id"], noise=d["noise"], n_frames=[9, 5]))
        got = _outs(model.forward_formant(d["units"], d["f0"], d["volume"], d["spk_id"], torch.ones(B, FR, device=dev),
                                          noise=d["noise"], n_frames=[9, 5]))
        assert all(torch.equal(a, b) for a, b in zip(got, ragged)) and float(want[0].abs().max()) > 1e-3


@pytest.mark.parametrize("counts", [None, [9, 5]], ids=["solo", "ragged"])
@pytest.mark.parametrize("what", ["+3 per row", "ramp"])
def test_forward_formant_is_the_eager_composition(model, dev, what, counts):
    d = _inputs(dev)
    if what == "ramp":
        factors = _f32(dev, [[FC.factor(-4 + i + 2 * b) for i in range(FR)] for b in range(B)])
        formant = factors
    else:
        factors, formant = torch.full((B,), float(FC.factor(3)), device=dev), 3
    kw = {} if counts is None else {"n_frames": counts}
    with torch.no_grad():
        got = _outs(model.forward_formant(d["units"], d["f0"], d["volume"], d["spk_id"], formant, noise=d["noise"], **kw))
        want = _composition(model, d, factors, counts)
        plain = model(d["units"], d["f0"], d["volume"], d["spk_id"], noise=d["noise"], **kw)[0]
    torch.cuda.synchronize()
    for name, a, b in zip(("signal", "phase", "harmonic", "noise"), got, want if len(want) == 4 else [want[0], want[1], want[0], want[0]]):
        print(f"{what}, {name}: largest difference {float((a - b).abs().max()):.3e}")
        assert torch.equal(a, b), name
    assert rms((got[0] - plain).cpu()) > 1e-4                                             # the shift is heard
    if what == "+3 per row":                                                               # a number is its factor as a tensor
        with torch.no_grad():
            again = model.forward_formant(d["units"], d["f0"], d["volume"], d["spk_id"], factors, noise=d["noise"], **kw)[0]
        assert torch.equal(again, got[0])
    if counts is not None:                                                                 # a ragged row is zero past its end
        assert not got[0][1, 5 * HOP:].any()


def test_per_frame_speaker_mix_is_accepted(model, dev):
    d = _inputs(dev)
    ids = _i32(dev, [[1, 2], [3, 1]])
    w = torch.rand(B, FR, 2, device=dev)
    with torch.no_grad():
        got = model.forward_formant(d["units"], d["f0"], d["volume"], None, 2, noise=d["noise"], spk_mix_rows=(ids, w))[0]
        same = model.forward_formant(d["units"], d["f0"], d["volume"], None, 0, noise=d["noise"], spk_mix_rows=(ids, w))[0]
        plain = model(d["units"], d["f0"], d["volume"], None, noise=d["noise"], spk_mix_rows=(ids, w))[0]
    assert torch.equal(same, plain) and rms((got - plain).cpu()) > 1e-4 and torch.isfinite(got).all()


def test_training_models_refuse(dev, lib_path):
    d = _inputs(dev)
    for kind in ("CombSub", "Sins", "CombSubFast"):
        m = bank_model(kind, 3, 43, dev).train()
        with torch.enable_grad():
            with pytest.raises(NotImplementedError, match="inference only"):
                m.forward_formant(d["units"], d["f0"], d["volume"], d["spk_id"], 2, noise=d["noise"])


# ---- 3. jobs --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(dev, lib_path):
    return [bank_model("CombSub", 2, 43, dev), bank_model("Sins", 2, 44, dev)]


def _noise(dev, slices, jobs, seed=915):
    import infer_offline
    pieces = infer_offline.piece_table(slices, float(HOP))
    rng = np.random.Generator(np.random.PCG64(seed))
    return [[torch.from_numpy(rng.random(row[2] * HOP, dtype=np.float32)).to(dev) for row in pieces if row[0] == job[0]] for job in jobs]


def test_jobs_with_a_formant_end_to_end(dev, lib_path, models, encoder, extractor):  # noqa: F811
    """Two files (1.3 s in two slices, 0.7 s), three jobs, every row a group of its own, injected noise.  Job 0 (Sins): no
    formant; job 1 (CombSub): +2 semitones; job 2 (CombSub): a timeline of two points whose slope crosses both slices."""
    import infer_offline
    from infer_offline import FormantTimeline
    audios, slices = _files()
    tl = FormantTimeline([(0.1, -3.0), (1.2, 4.0)])
    jobs = [(1, 1, 2, 3.0), (0, 0, 1, 0.0, 2), (0, 0, 1, -1.0, tl)]
    noise = _noise(dev, slices, jobs)
    run = lambda jj: infer_offline.convert_many_device(None, _args(), audios, SR, encoder, extractor, slices=slices, jobs=jj,  # noqa: E731
                                                       models=models, batch_frames=1, noise=noise)
    got, spans, sr_o = run(jobs)
    ref, ref_spans, _ = run([job[:4] for job in jobs])
    torch.cuda.synchronize()
    ctx = infer_offline.hipddsp.context_for(dev)
    ctx.poll_error()
    assert spans == ref_spans and sr_o == SR
    span = lambda x, j: x[spans[j][0]:spans[j][0] + spans[j][1]]  # noqa: E731
    # the job without a formant, on a model without one among its jobs: the parent path's bits
    assert torch.equal(span(got, 0), span(ref, 0)) and float(span(ref, 0).abs().max()) > 1e-3
    files = infer_offline.analyse_many(_args(), audios, SR, slices, encoder, extractor, 0, None)
    at, semi = tl.frames(SR, HOP)
    assert at == [9, 103] and [row[1] for row in files["pieces"] if row[0] == 0] == [0, 77]
    n = files["f0"].shape[1]
    for j, points in ((1, [(0, 2.0)]), (2, list(zip(at, semi)))):
        k, m, spk, key = jobs[j][:4]
        times, keys = [p[0] for p in points], np.array([p[1] for p in points], dtype=np.float32)
        factor, _ = KC.factors(times, keys, [KC.stored_factor(p[1]) for p in points], np.arange(n, dtype=np.float64))
        # the factor rows the render builds: `pieces_gather(key_timeline=)` over an f0 of ones, bit for bit the statement's
        tabs = tuple(t.to(dev) for t in infer_offline.formant_tables(infer_offline.job_formants(jobs), SR, HOP))
        rows = [row + (j,) for row in files["pieces"] if row[0] == k]
        _, fac, _ = ctx.pieces_gather(_i32(dev, rows), files["n_samples_dev"], files["n_frames_dev"], f0=torch.ones_like(files["f0"]),
                                      N_max=max(r[2] for r in rows), key_timeline=tabs)
        segments, f0, volume = infer_offline.file_features(files, k)
        shifted = f0[:, :n] * float(2 ** (key / 12))
        spk_id = torch.tensor([[spk]], dtype=torch.int64, device=dev)
        outs = []
        for i, ((start, units), row) in enumerate(zip(segments, rows)):
            cnt = units.shape[1]
            assert np.array_equal(fac[i, :cnt].cpu().numpy(), factor[start:start + cnt]) and not fac[i, cnt:].any()
            sl = slice(start, start + cnt)
            with torch.no_grad():
                sig = models[m].forward_formant(units, shifted[:, sl], volume[:, sl], spk_id, _f32(dev, factor[None, sl]),
                                                noise=noise[j][i][None])[0]
            ctx.volume_gate_rows_(sig, files["volume"], _i32(dev, [start]), _i32(dev, [cnt]), -60, HOP,
                                  file_dev=_i32(dev, [k]), file_frames_dev=files["n_frames_dev"])
            outs.append(sig[:, :cnt * HOP])
        plan = infer_offline.stitch_plan_many([[r[1] for r in rows]], [[o.shape[-1] for o in outs]], HOP, SR, SR)
        want = ctx.stitch(outs, plan[1], plan[2], plan[3])
        e = rms((span(got, j) - want).cpu())
        print(f"job {j} against the per-slice eager render through forward_formant: rms {e:.3e}")
        assert want.numel() == spans[j][1] and e < GATE and float(want.abs().max()) > 1e-3
        assert rms((span(got, j) - span(ref, j)).cpu()) > 1e-3                              # the shift is heard


# ---- 4. the bank ----------------------------------------------------------------------------------------------------------------
S, K = 3, 3
BLOCK_TIME, XFADE_TIME, BUFFER_NUM, THR = 0.1, 0.04, 4, -45.0       # the geometry of tests/test_gpu_bank_glide.py


@pytest.fixture(scope="module")
def bank_synth(dev, lib_path):
    return synthetic.build_model("CombSub", seed=43, device=dev)[0]


def _bank(model, dev, **kw):
    import realtime
    return realtime.StreamBank(model, S, SR, BLOCK_TIME, XFADE_TIME, dev, buffer_num=BUFFER_NUM, threshold_db=THR, max_mix=K, **kw)


def _block(k, bank, dev):
    rng = np.random.Generator(np.random.PCG64(700 + k))
    t = (np.arange(bank.block) + k * bank.block) / SR
    blocks = np.stack([0.2 * np.sin(2 * np.pi * f * t) + 0.01 * rng.standard_normal(bank.block) for f in (147.0, 220.0, 330.0)])
    z = synthetic.make_inputs(8100 + k, S, bank.frames)
    return {"blocks": torch.from_numpy(blocks.astype(np.float32)).to(dev), "units": z["units"].to(dev), "f0": z["f0"].to(dev),
            "noise": z["noise"].to(dev)}


def _push(bank, x, active=None):
    row = (lambda name: x[name]) if active is None else (lambda name: x[name][list(active)].contiguous())
    return bank.push_block(row("blocks"), row("units"), row("f0"), noise=row("noise"), **({} if active is None else {"active": active}))


def test_bank_formant_row(dev, bank_synth):
    import hipddsp
    model = bank_synth
    plain, bank, eager = _bank(model, dev), _bank(model, dev, formant=True), _bank(model, dev, formant=True, use_graph=False)
    assert plain.graph_builds == bank.graph_builds == 1 and eager.graph_builds == 0
    ctx = hipddsp.context_for(dev)
    for k in range(4):
        if k == 2:
            bank.set_formant(1, 4)
            eager.set_formant(1, 4)
        x = _block(k, plain, dev)
        a, b, c = _push(plain, x), _push(bank, x), _push(eager, x)
        torch.cuda.synchronize()
        assert torch.equal(b, c) and torch.equal(bank.last_signal, eager.last_signal), k
        if k < 2:                                                                          # all rows at 1: the plain bank's bits
            assert torch.equal(a, b) and torch.equal(plain.last_signal, bank.last_signal), k
            continue
        assert torch.equal(bank.last_signal[[0, 2]], plain.last_signal[[0, 2]]) and torch.equal(a[[0, 2]], b[[0, 2]]), k
        factors = torch.tensor([1.0, 2 ** (4.0 / 12), 1.0], dtype=torch.float32).to(dev)
        assert torch.equal(bank.formant, factors)
        with torch.no_grad():
            sig = model.forward_formant(bank.last_units, bank.last_f0, bank.last_volume, None, factors,
                                        spk_mix_rows=(bank.spk_ids, bank.spk_w), noise=x["noise"])[0]
        ctx.volume_gate_(sig, bank.last_volume, THR, 512)
        torch.cuda.synchronize()
        assert torch.equal(bank.last_signal, sig), (k, float((bank.last_signal - sig).abs().max()))
        assert rms((bank.last_signal[1] - plain.last_signal[1]).cpu()) > 1e-4
    assert bank.graph_builds == 1 and eager.graph_builds == 0                              # `set_formant` captured nothing
    bank.reset(1)
    assert bank.formant.tolist() == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match="formant=True with models="):
        _bank(None, dev, models=[model, model], formant=True)


def test_bank_formant_with_active_widths(dev, bank_synth):
    """`active_widths=(1, 2)` and the slots 2 and 0 in one call (`active` names them in increasing order, [0, 2], as every call
    must).  The paused slot 1 keeps its formant row and its window; a compact row reads its SLOT's factor through the width's
    row table: the block equals the eager `forward_formant` with the two slots' factors."""
    import hipddsp
    model = bank_synth
    bank = _bank(model, dev, formant=True, active_widths=(1, 2))
    builds, ctx = bank.graph_builds, hipddsp.context_for(dev)
    bank.set_formant(1, -5)
    bank.set_formant(2, 3)
    with pytest.raises(ValueError, match="strictly increasing"):
        _push(bank, _block(0, bank, dev), active=[2, 0])
    kept = [bank.formant.clone(), bank.windows[1].clone()]
    for k in range(2):
        x = _block(k, bank, dev)
        _push(bank, x, active=[0, 2])
        torch.cuda.synchronize()
        assert torch.equal(bank.formant, kept[0]) and torch.equal(bank.windows[1], kept[1]), k
        with torch.no_grad():
            sig = model.forward_formant(bank.last_units, bank.last_f0, bank.last_volume, None, bank.formant[[0, 2]].contiguous(),
                                        spk_mix_rows=(bank.spk_ids[[0, 2]].contiguous(), bank.spk_w[[0, 2]].contiguous()),
                                        noise=x["noise"][[0, 2]].contiguous())[0]
            same = model(bank.last_units, bank.last_f0, bank.last_volume, None, noise=x["noise"][[0, 2]].contiguous(),
                         spk_mix_rows=(bank.spk_ids[[0, 2]].contiguous(), bank.spk_w[[0, 2]].contiguous()))[0]
        ctx.volume_gate_(sig, bank.last_volume, THR, 512)
        ctx.volume_gate_(same, bank.last_volume, THR, 512)
        torch.cuda.synchronize()
        assert bank.last_signal.shape[0] == 2 and torch.equal(bank.last_signal, sig), k
        assert torch.equal(sig[0], same[0]) and rms((sig[1] - same[1]).cpu()) > 1e-4         # slot 0 at 1, slot 2 shifted
    assert bank.graph_builds == builds
