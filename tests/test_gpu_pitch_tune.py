"""Pitch correction on the device: `ddsp_f0_tune` against its numpy statement (tests/pitch_tune_cases.py), offline jobs with a
tune, and `StreamBank(tune=True)`.

Bounds.  `corr` against the statement's c: 1e-12 semitones.  |c| <= 6, one composition of the scan rounds to some 1e-15, a
frame's value passes through at most log2(64) = 6 of them in a step and one carry per 64 frames, and the device's log2 moves m
by an ulp of a number below 128 (1.4e-14): some 1e-13 in all.  For the alpha == 1 owner every A is exactly 0, the products are
exact zeros and c is d: bit for bit (the count of differing frames and the largest difference are printed first).  The output f0: 1 fp32 ulp from the statement rounded to fp32 - the scan error is eight
orders below an ulp; what remains is the device's log2 and exp2 against numpy's next to a rounding boundary.  Elements the
rule leaves alone: their bits.  A job against the per-slice eager render whose f0 is the gather and then the statement on the
host: rms < `GATE` = 1e-4, the gate of the jobs path elsewhere (a one-ulp move of f0 changes the phase integral)."""
import numpy as np
import pytest
import torch

import pitch_tune_cases as PC
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


def _f64(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------------
def _run(ctx, dev, f0, masks, params, counts=None, owner=None, corr=True):
    got = _f32(dev, f0)
    c = torch.full(got.shape, 7.0, dtype=torch.float64, device=dev) if corr else None       # (7: no c_t; every element is written)
    out = ctx.f0_tune_(got, _i32(dev, masks), _f64(dev, params), n_frames=None if counts is None else _i32(dev, counts),
                       owner=None if owner is None else _i32(dev, owner), corr=c)
    assert out is got
    torch.cuda.synchronize()
    return got.cpu().numpy(), None if c is None else c.cpu().numpy()


def _hold(f0, got, corr, want, want_corr, masks, params, counts, owner, what):
    """The four checks of the module docstring on one call."""
    B, Fr = f0.shape
    touched = np.zeros((B, Fr), dtype=bool)
    for b in range(B):
        j = b if owner is None else int(owner[b])
        if 0 <= j < len(masks) and masks[j] & 0xfff and not PC.bad_setting(*params[j]) and params[j][1] != 0:
            n = Fr if counts is None else int(counts[b])
            touched[b, :n] = np.isfinite(f0[b, :n]) & (f0[b, :n] > 0)
            if params[j][2] == 1.0 and touched[b].any():
                exact = np.abs(corr[b] - want_corr[b])
                print(f"{what}, row {b} (alpha 1): {int((exact != 0).sum())} of {int(touched[b].sum())} c differ, largest {exact.max():.3e}")
                assert np.array_equal(corr[b], want_corr[b])
    assert PC.same_bits(got[~touched], f0[~touched]) and PC.same_bits(want[~touched], f0[~touched])
    assert not corr[~touched].any() and not np.signbit(corr[~touched]).any()
    if touched.any():
        e_c = np.abs(corr - want_corr)[touched].max()
        ulps = PC.ulps32(got[touched], want[touched])
        print(f"{what}: {int(touched.sum())} frames corrected, corr off by at most {e_c:.3e} semitones, f0 by at most "
              f"{int(ulps.max())} ulp ({int((ulps != 0).sum())} frames differ)")
        assert e_c <= 1e-12 and ulps.max() <= 1
        assert np.abs(want_corr[touched]).max() <= 6.0


@pytest.mark.parametrize("Fr", PC.SHAPES)
def test_kernel_matches_the_statement(ctx, dev, lib_path, Fr):
    f0, gaps = PC.rows(Fr)
    counts = PC.counts(Fr)
    ctx.poll_error()
    moved = 0
    for owner in PC.OWNERS:
        for n in (None, counts):
            want, want_corr, err = PC.tune_rows(f0, PC.MASKS, PC.PARAMS, n, owner)
            got, corr = _run(ctx, dev, f0, PC.MASKS, PC.PARAMS, n, owner)
            assert not err
            _hold(f0, got, corr, want, want_corr, PC.MASKS, PC.PARAMS, n, owner, f"Fr {Fr}, owner {owner.tolist()}, counts {n is not None}")
            moved += int((got.view(np.uint32) != f0.view(np.uint32)).sum())
            # without corr: the same f0
            assert PC.same_bits(_run(ctx, dev, f0, PC.MASKS, PC.PARAMS, n, owner, corr=False)[0], got)
    assert moved > 0 or Fr == 1
    # owner None: row b takes setting b (five rows, six settings)
    want, want_corr, err = PC.tune_rows(f0, PC.MASKS[[1, 2, 0, 4, 5]], PC.PARAMS[[1, 2, 0, 4, 5]], counts)
    got, corr = _run(ctx, dev, f0, PC.MASKS[[1, 2, 0, 4, 5]], PC.PARAMS[[1, 2, 0, 4, 5]], counts)
    _hold(f0, got, corr, want, want_corr, PC.MASKS[[1, 2, 0, 4, 5]], PC.PARAMS[[1, 2, 0, 4, 5]], counts, None, f"Fr {Fr}, no owner table")
    # ... and fewer settings than rows: the rows behind them are padding
    got, corr = _run(ctx, dev, f0, PC.MASKS[[1, 2]], PC.PARAMS[[1, 2]], counts)
    assert PC.same_bits(got[2:], f0[2:]) and not corr[2:].any()
    ctx.poll_error()                                                                      # none of this raised the error word


def test_exact_ties_take_the_lower_note(ctx, dev, lib_path):
    """Mask {G, B}, a4 = 440: 220, 440 and 880 Hz are A3, A4, A5, midway between G and B - log2 of a power of two is exact."""
    f0 = np.array([[220.0, 440.0, 880.0]], dtype=np.float32)
    masks, params = np.array([PC.G_B], dtype=np.int32), np.array([[440.0, 1.0, 1.0]])
    got, corr = _run(ctx, dev, f0, masks, params)
    want, want_corr, _ = PC.tune_rows(f0, masks, params)
    assert corr.tolist() == want_corr.tolist() == [[-2.0, -2.0, -2.0]]
    assert PC.ulps32(got, want).max() <= 1 and np.allclose(got, f0 * 2 ** (-2 / 12), rtol=1e-6)


def test_a_bad_setting_leaves_its_rows_and_sets_the_error_word(ctx, dev, lib_path):
    """An error path that returns: no address depends on the setting."""
    f0, _ = PC.rows(65, seed=3)
    owner = np.array([1, 3, 2, 3, 0], dtype=np.int32)
    for j, column, value in PC.BAD:
        torch.cuda.synchronize()
        ctx.poll_error()
        params = PC.PARAMS.copy()
        params[j, column] = value
        want, want_corr, err = PC.tune_rows(f0, PC.MASKS, params, None, owner)
        got, corr = _run(ctx, dev, f0, PC.MASKS, params, None, owner)
        assert err and PC.same_bits(got[[1, 3, 4]], f0[[1, 3, 4]]) and not corr[[1, 3, 4]].any()
        assert not PC.same_bits(got[[0, 2]], f0[[0, 2]]) and PC.ulps32(got[[0, 2]], want[[0, 2]]).max() <= 1
        with pytest.raises(ValueError, match="ddsp_f0_tune"):
            ctx.poll_error()
        ctx.poll_error()                                                                  # read and cleared: reported once
        # the bad setting behind no row, and behind a mask of no bits: nobody judges it
        _run(ctx, dev, f0, PC.MASKS, params, None, np.array([1, 2, 2, 1, 0], dtype=np.int32))
        masks = PC.MASKS.copy()
        masks[j] = 0
        assert PC.same_bits(_run(ctx, dev, f0, masks, params, None, owner)[0][[1, 3]], f0[[1, 3]])
        ctx.poll_error()


def test_one_run_under_capture_equals_the_eager_run(ctx, dev, lib_path):
    f0, _ = PC.rows(130, seed=5)
    owner, counts = PC.OWNERS[1], PC.counts(130)
    eager, eager_corr = _run(ctx, dev, f0, PC.MASKS, PC.PARAMS, counts, owner)
    static, corr = _f32(dev, f0), torch.zeros(PC.B, 130, dtype=torch.float64, device=dev)
    args = (_i32(dev, PC.MASKS), _f64(dev, PC.PARAMS))
    kw = {"n_frames": _i32(dev, counts), "owner": _i32(dev, owner), "corr": corr}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ctx.f0_tune_(static, *args, **kw)
    torch.cuda.synchronize()
    static.copy_(_f32(dev, f0))                                       # (the capture itself launched nothing)
    graph.replay()
    torch.cuda.synchronize()
    assert PC.same_bits(static.cpu().numpy(), eager) and PC.same_bits(corr.cpu().numpy(), eager_corr)
    ctx.poll_error()


# ---- 2. jobs --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(dev, lib_path):
    return [bank_model("CombSub", 2, 43, dev), bank_model("Sins", 2, 44, dev)]


def _noise(dev, slices, jobs, seed=917):
    import infer_offline
    pieces = infer_offline.piece_table(slices, float(HOP))
    rng = np.random.Generator(np.random.PCG64(seed))
    return [[torch.from_numpy(rng.random(row[2] * HOP, dtype=np.float32)).to(dev) for row in pieces if row[0] == job[0]] for job in jobs]


class _EnhancerStub:
    """Keeps the f0 rows it is handed and returns the signal as it came."""

    def __init__(self):
        self.seen = []

    def enhance_batch(self, wav, sr, f0, block, counts, adaptive_key=0, n_f0=None):
        self.seen += [f0[i, :n, 0].clone() for i, n in enumerate(n_f0)]
        return wav, sr, list(counts)


def test_jobs_with_a_tune_end_to_end(dev, lib_path, models, encoder, extractor, monkeypatch):  # noqa: F811
    """Two files (1.3 s in two slices, 0.7 s), three jobs, every row a group of its own, injected noise.  Job 0 (Sins): no tune;
    job 1 (CombSub): A minor at 30 ms; job 2 (CombSub): a C major pentatonic hard tune behind a key timeline."""
    import hipddsp
    import infer_offline
    from infer_offline import KeyTimeline, PitchTune
    audios, slices = _files()
    tunes = [None, PitchTune.scale("A", "minor", retune=0.03), PitchTune.scale("C", "major_pentatonic", strength=0.9, retune=0)]
    jobs = [(1, 1, 2, 3.0), (0, 0, 1, 0.0, None, tunes[1]), (0, 0, 1, KeyTimeline([(0.1, -2.0), (1.2, 3.0)]), None, tunes[2])]
    noise = _noise(dev, slices, jobs)
    handed = []                                                        # every f0 the kernel returned, with its row's job and count
    launch = hipddsp.Context.f0_tune_

    def counted(self, f0, mask, param, n_frames=None, owner=None, corr=None):
        out = launch(self, f0, mask, param, n_frames=n_frames, owner=owner, corr=corr)
        handed.extend((int(j), int(n), out[i, :int(n)].clone()) for i, (j, n) in enumerate(zip(owner.tolist(), n_frames.tolist())))
        return out
    monkeypatch.setattr(hipddsp.Context, "f0_tune_", counted)
    run = lambda jj, **kw: infer_offline.convert_many_device(None, _args(), audios, SR, encoder, extractor, slices=slices, jobs=jj,  # noqa: E731
                                                             models=models, batch_frames=1, noise=noise, **kw)
    ref, ref_spans, _ = run([job[:4] for job in jobs])
    assert not handed                                                  # without a tune among the jobs nothing is launched
    got, spans, sr_o = run(jobs)
    torch.cuda.synchronize()
    ctx = hipddsp.context_for(dev)
    ctx.poll_error()
    assert spans == ref_spans and sr_o == SR and len(handed) == 5
    span = lambda x, j: x[spans[j][0]:spans[j][0] + spans[j][1]]  # noqa: E731
    assert torch.equal(span(got, 0), span(ref, 0)) and float(span(ref, 0).abs().max()) > 1e-3   # the untuned job keeps its bits
    files = infer_offline.analyse_many(_args(), audios, SR, slices, encoder, extractor, 0, None)
    key_tabs = tuple(t.to(dev) for t in infer_offline.key_tables([job[3] for job in jobs], SR, HOP))
    masks, params = infer_offline.tune_tables(tunes, SR, HOP)
    for j in (1, 2):
        k, m, spk = jobs[j][:3]
        rows = [row + (j,) for row in files["pieces"] if row[0] == k]
        _, shifted, _ = ctx.pieces_gather(_i32(dev, rows), files["n_samples_dev"], files["n_frames_dev"], f0=files["f0"],
                                          N_max=max(r[2] for r in rows), key_timeline=key_tabs)
        segments, _, volume = infer_offline.file_features(files, k)
        spk_id = torch.tensor([[spk]], dtype=torch.int64, device=dev)
        outs = []
        for i, ((start, units), row) in enumerate(zip(segments, rows)):
            cnt = units.shape[1]
            before = shifted[i:i + 1, :cnt].cpu().numpy()
            tuned, corr, err = PC.tune_rows(before, masks.numpy()[[j]], params.numpy()[[j]])
            assert not err and np.abs(corr).max() > 0.05 and np.abs(corr).max() <= 6
            with torch.no_grad():
                sig = models[m](units, _f32(dev, tuned)[:, :, None], volume[:, start:start + cnt], spk_id, noise=noise[j][i][None])[0]
            ctx.volume_gate_rows_(sig, files["volume"], _i32(dev, [start]), _i32(dev, [cnt]), -60, HOP,
                                  file_dev=_i32(dev, [k]), file_frames_dev=files["n_frames_dev"])
            outs.append(sig[:, :cnt * HOP])
            mine = [f for jj, n, f in handed if jj == j and n == cnt]
            ulps = PC.ulps32(mine[0].cpu().numpy(), tuned[0])
            print(f"job {j} slice {i}: f0 of the call against the statement on the host: at most {int(ulps.max())} ulp")
            assert len(mine) == 1 and ulps.max() <= 1
        plan = infer_offline.stitch_plan_many([[r[1] for r in rows]], [[o.shape[-1] for o in outs]], HOP, SR, SR)
        want = ctx.stitch(outs, plan[1], plan[2], plan[3])
        e = rms((span(got, j) - want).cpu())
        print(f"job {j} against the per-slice eager render over the statement's f0: rms {e:.3e}")
        assert want.numel() == spans[j][1] and e < GATE and float(want.abs().max()) > 1e-3
        assert rms((span(got, j) - span(ref, j)).cpu()) > 1e-3                              # the correction is heard
    # the enhancer sees the render's f0: the same kernel on the same rows, bit for bit
    render = list(handed)
    del handed[:]
    stub = _EnhancerStub()
    again, _, _ = run(jobs, enhancer=stub)
    torch.cuda.synchronize()
    assert torch.equal(again, got) and len(handed) == 10 and len(stub.seen) == 5
    by_row = {(j, n): f for j, n, f in handed[:5]}
    assert len(by_row) == 5 and all(torch.equal(by_row[(j, n)], f) for j, n, f in render + handed[5:])
    assert all(any(f.numel() == g.numel() and torch.equal(f, g) for _, _, g in handed[:5]) for f in stub.seen)


# ---- 3. the bank ----------------------------------------------------------------------------------------------------------------
S, K = 3, 3
BLOCK_TIME, XFADE_TIME, BUFFER_NUM, THR = 0.1, 0.04, 4, -45.0       # the geometry of tests/test_gpu_formant.py


def _bank(model, dev, encoder, **kw):  # noqa: F811
    import realtime
    return realtime.StreamBank(model, S, SR, BLOCK_TIME, XFADE_TIME, dev, buffer_num=BUFFER_NUM, threshold_db=THR, max_mix=K,
                               units_encoder=encoder, f0_extractor="ac", f0_min=65, f0_max=800, f0_dither=False, **kw)


def _block(k, bank, dev):
    """Three sung tones off the grid of A = 440: 150, 215 and 335 Hz."""
    rng = np.random.Generator(np.random.PCG64(720 + k))
    t = (np.arange(bank.block) + k * bank.block) / SR
    blocks = np.stack([0.2 * np.sin(2 * np.pi * f * t) + 0.005 * rng.standard_normal(bank.block) for f in (150.0, 215.0, 335.0)])
    z = synthetic.make_inputs(8200 + k, S, bank.frames)
    return {"blocks": torch.from_numpy(blocks.astype(np.float32)).to(dev), "noise": z["noise"].to(dev)}


def _push(bank, x, active=None):
    row = (lambda name: x[name]) if active is None else (lambda name: x[name][list(active)].contiguous())
    return bank.push_audio(row("blocks"), noise=row("noise"), **({} if active is None else {"active": active}))


def test_bank_tune_rows(dev, lib_path, encoder):  # noqa: F811
    from infer_offline import PitchTune
    model = synthetic.build_model("CombSub", seed=43, device=dev)[0]
    plain, bank, eager = _bank(model, dev, encoder), _bank(model, dev, encoder, tune=True), _bank(model, dev, encoder, tune=True, use_graph=False)
    assert plain.graph_builds == bank.graph_builds == 1 and eager.graph_builds == 0
    tune = PitchTune.scale("A", "minor", retune=0.02)
    moved = 0.0
    for k in range(5):
        if k == 3:
            bank.set_tune(1, tune)
            eager.set_tune(1, tune)
        x = _block(k, plain, dev)
        a, b, c = _push(plain, x), _push(bank, x), _push(eager, x)
        torch.cuda.synchronize()
        assert torch.equal(b, c) and torch.equal(bank.last_signal, eager.last_signal) and torch.equal(bank.last_f0, eager.last_f0), k
        if k < 3:                                                                          # nothing set: the plain bank's bits
            assert torch.equal(a, b) and torch.equal(plain.last_signal, bank.last_signal) and torch.equal(plain.last_f0, bank.last_f0), k
            continue
        assert torch.equal(bank.last_signal[[0, 2]], plain.last_signal[[0, 2]]) and torch.equal(a[[0, 2]], b[[0, 2]]), k
        assert torch.equal(bank.last_f0[[0, 2]], plain.last_f0[[0, 2]]), k
        # slot 1's f0 is the statement on the plain bank's
        mask, param = tune.setting(bank.hop_size / SR)
        want, corr, _ = PC.tune_rows(plain.last_f0[1:2, :, 0].cpu().numpy(), [mask], [param])
        assert PC.ulps32(bank.last_f0[1, :, 0].cpu().numpy(), want[0]).max() <= 1
        moved = max(moved, float(np.abs(corr).max()), 0.0)
        assert rms((bank.last_signal[1] - plain.last_signal[1]).cpu()) > 1e-4
    assert moved > 0.1 and bank.graph_builds == 1 and eager.graph_builds == 0              # `set_tune` captured nothing
    assert bank.tune_mask.tolist() == [0, tune.mask, 0]
    bank.reset(1)
    assert bank.tune_mask.tolist() == [0, 0, 0] and bank.graph_builds == 1
    x = _block(5, plain, dev)
    bank.set_tune(1, tune)
    bank.set_tune(1, None)
    plain.reset(1)
    assert torch.equal(_push(plain, x), _push(bank, x)) and bank.graph_builds == 1


def test_bank_tune_with_active_widths(dev, lib_path, encoder):  # noqa: F811
    """`active_widths=(2,)`: the slots [0, 2] fill the compact width, slot 2 alone leaves it a padding row.  A compact row reads its SLOT's setting through the width's row table: the graph
    path equals the eager chain, the untuned slot equals the bank without the feature."""
    from infer_offline import PitchTune
    model = synthetic.build_model("CombSub", seed=43, device=dev)[0]
    kw = dict(active_widths=(2,))
    plain, bank, eager = _bank(model, dev, encoder, **kw), _bank(model, dev, encoder, tune=True, **kw), \
        _bank(model, dev, encoder, tune=True, use_graph=False, **kw)
    builds = bank.graph_builds
    for b in (bank, eager):
        b.set_tune(2, PitchTune(["C", "E", "G"], strength=0.7, retune=0.01))
    for k, active in enumerate(([0, 2], [2], [0, 2], [2])):                                # ([2] at width 2: a padding row)
        x = _block(k, plain, dev)
        a, b, c = _push(plain, x, active), _push(bank, x, active), _push(eager, x, active)
        torch.cuda.synchronize()
        assert torch.equal(b, c) and torch.equal(bank.last_f0, eager.last_f0) and b.shape[0] == len(active), k
        if len(active) == 2:
            assert torch.equal(a[0], b[0]) and torch.equal(plain.last_f0[0], bank.last_f0[0]), k
        assert not torch.equal(plain.last_f0[-1], bank.last_f0[-1]) and torch.isfinite(b).all(), k
    assert bank.graph_builds == builds
    import hipddsp
    hipddsp.context_for(dev).poll_error()


def test_bank_tune_with_models(dev, lib_path, encoder):  # noqa: F811
    """The correction sits in the shared analysis: a bank with `models=` takes it, and a slot's f0 is what the single-model
    bank's is."""
    from infer_offline import PitchTune
    import realtime
    m0, m1 = bank_model("CombSub", 2, 43, dev), bank_model("Sins", 2, 44, dev)
    two = _bank(None, dev, encoder, models=[m0, m1], tune=True)
    one = _bank(m0, dev, encoder, tune=True)
    builds = two.graph_builds
    two.set_model(1, 1)
    tune = PitchTune.scale("D", "major", retune=0.02)
    for b in (one, two):
        b.set_tune(1, tune)
        b.set_tune(2, tune)
    for k in range(3):
        x = _block(k, one, dev)
        got, want = _push(two, x), _push(one, x)
        torch.cuda.synchronize()
        assert torch.equal(two.last_f0, one.last_f0) and torch.isfinite(got).all() and float(got.abs().max()) > 0, k
    assert two.graph_builds == builds
    with pytest.raises(ValueError, match="without tune=True"):
        realtime.StreamBank.set_tune(_bank(m0, dev, encoder), 0, tune)
