"""Key timelines on the device: `ddsp_pieces_gather_keys` and `ddsp_bank_key_glide` against the fp64 numpy statement of the
rule (tests/key_timeline_cases.py), jobs with a moving key through `convert_many_device`, and `StreamBank(pitch_breakpoints=)`.

Exactness.  Where the rule owes a STORED factor (before the first breakpoint, behind the last, on a breakpoint, between two of
equal semitones, a numeric key, a slot without a timeline, a padding row) the kernels owe the statement's bits.  On a slope the
factor is an fp64 exp2 rounded to fp32: it can differ from numpy's only where the fp64 values round apart at a near-tie, 1 fp32
ulp; a general f0 times it adds the product's own rounding, 2 ulps.  Signals: a job against the per-slice eager render is held
to rms < 1e-4 (`GATE`, as tests/test_gpu_many_jobs.py holds the jobs path), the enhancer case to rms <= 1e-4
(tests/test_gpu_many.py's enhancer test), the bank against its eager chain bit for bit (tests/test_gpu_bank_glide.py)."""
import numpy as np
import pytest
import torch

import key_timeline_cases as KC
import synthetic
from conftest import rms
from test_bank_models_host import bank_model
from test_gpu_many import GATE, _fixed_enhancer
from test_gpu_many import encoder  # noqa: F401  (the module-scoped random-weight HubertSoft fixture)
from test_gpu_many_jobs import _args, _files, extractor  # noqa: F401

pytestmark = pytest.mark.gpu
SR, HOP = synthetic.SR, synthetic.HOP


def _i32(dev, a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev)


def _tabs(dev, tabs):
    return tuple(torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in tabs)


# ---- 1. the gather --------------------------------------------------------------------------------------------------------------
N_SAMPLES, N_FRAMES, N_MAX, S_MAX = [900, 1201], [37, 30], 24, 700
# job 0: a numeric key; 1: a slope 8 -> 30 with a breakpoint at 16, inside the pieces; 2: three points wholly before the pieces;
# 3: two points of equal semitones (and a slope behind them)
KEY_JOBS = [3.0, [(2, -2.0), (16, 1.5), (30, 4.0)], [(0, 1.0), (2, 5.0), (3, -7.0)], [(1, 2.5), (20, 2.5), (36, 0.0)]]
# (file, start_frame, n_frames, start_sample, n_samples, job): file 1's f0 is all 1.0, so its rows show the factor itself.
# Starts 4, 8 and 12 are multiples of 4 (16-byte loads), start 5 is not; n_frames 24 = N_max, the others leave a zero tail.
ROWS = [(0, 4, 24, 96, 600, 1), (0, 5, 19, 120, 700, 1), (1, 8, 22, 0, 1, 1), (1, 5, 24, 0, 1, 3), (0, 12, 24, 300, 500, 3),
        (0, 5, 21, 7, 333, 2), (1, 4, 20, 0, 1, 2), (0, 8, 17, 0, 4, 0), (1, 5, 9, 3, 5, 0)]


def _gather_case(dev):
    rng = np.random.Generator(np.random.PCG64(2718))
    nan = float("nan")
    audio, f0, volume = np.full((2, 1201), nan, np.float32), np.full((2, 37), nan, np.float32), np.full((2, 37), nan, np.float32)
    for k, (n, fr) in enumerate(zip(N_SAMPLES, N_FRAMES)):
        audio[k, :n] = rng.standard_normal(n).astype(np.float32)
        f0[k, :fr] = rng.uniform(80.0, 700.0, fr).astype(np.float32) if k == 0 else 1.0
        volume[k, :fr] = rng.random(fr).astype(np.float32)
    return audio, f0, volume


def _gather(ctx, dev, case, rows, tabs, **kw):
    audio, f0, volume = (torch.from_numpy(x).to(dev) for x in case)
    return ctx.pieces_gather(_i32(dev, rows), _i32(dev, N_SAMPLES), _i32(dev, N_FRAMES), audio=audio, S_max=S_MAX, f0=f0, volume=volume,
                             N_max=N_MAX, **kw)


def test_gather_matches_the_statement(ctx, dev, lib_path):
    case = _gather_case(dev)
    tabs = KC.tables(KEY_JOBS)
    assert tabs[0].tolist() == [0, 1, 4, 7, 10]
    wav, f0_rows, vol_rows = _gather(ctx, dev, case, ROWS, tabs, key_timeline=_tabs(dev, tabs))
    torch.cuda.synchronize()
    ctx.poll_error()
    want, stored, bad = KC.gather_f0(case[1], N_FRAMES, ROWS, tabs, N_MAX)
    got = f0_rows.cpu().numpy()
    assert not bad.any() and got.shape == want.shape == (len(ROWS), N_MAX)
    d = KC.ulps(got, want)
    for r, row in enumerate(ROWS):
        print(f"row {r} {row}: {int(stored[r, :row[2]].sum())} of {row[2]} frames owed exactly, largest distance {d[r].max():.2f} ulp")
        assert not got[r, row[2]:].any() and not np.signbit(got[r, row[2]:]).any(), r          # exact zeros behind n_frames
    # the stored-factor cases: one rounded product of fl32(f0) and bp_fac, bit for bit
    assert np.array_equal(got[stored], want[stored])
    assert stored[5, :21].all() and stored[6, :20].all() and stored[7, :17].all() and stored[8, :9].all()   # before, numeric
    assert stored[3, :16].all() and not stored[3, 16:].any() and stored[4, :9].all()                          # equal semitones
    assert stored[0, 12] and not stored[0, :12].any() and not stored[0, 13:].any()                            # on the breakpoint
    assert np.array_equal(got[6, :20], np.full(20, KC.stored_factor(-7.0))) and np.array_equal(got[8, :9], np.full(9, KC.stored_factor(3.0)))
    assert np.array_equal(got[3, :16], np.full(16, KC.stored_factor(2.5)))
    # slopes: the factor itself (f0 = 1) within 1 ulp, a general f0 within 2
    ones = [r for r, row in enumerate(ROWS) if row[0] == 1]
    assert d[ones].max() <= 1 and d.max() <= 2, (d[ones].max(), d.max())
    assert (np.diff(got[2, :22]) > 0).all() and (np.diff(got[3, 15:24]) < 0).all()                           # and they do move
    # audio and volume: the jobs gather's bits; with numeric keys only, the f0 rows too
    numeric = [3.0, -2.0, 0, 2.5]
    factor = torch.tensor([2 ** (float(k) / 12) for k in numeric], dtype=torch.float32).to(dev)
    old = _gather(ctx, dev, case, ROWS, None, key_factor=factor)
    assert torch.equal(wav, old[0]) and torch.equal(vol_rows, old[2]) and not torch.equal(f0_rows, old[1])
    new = _gather(ctx, dev, case, ROWS, None, key_timeline=_tabs(dev, KC.tables(numeric)))
    for a, b in zip(new, old):
        assert torch.equal(a, b)
    # the f0 rows alone (as the enhancer takes them)
    f0_dev = torch.from_numpy(case[1]).to(dev)
    alone = ctx.pieces_gather(_i32(dev, ROWS), _i32(dev, N_SAMPLES), _i32(dev, N_FRAMES), f0=f0_dev, N_max=N_MAX,
                              key_timeline=_tabs(dev, tabs))
    assert alone[0] is None and alone[2] is None and torch.equal(alone[1], f0_rows)
    torch.cuda.synchronize()
    ctx.poll_error()
    with pytest.raises(ValueError, match="key_timeline"):
        _gather(ctx, dev, case, ROWS, None, key_timeline=_tabs(dev, tabs), key_factor=factor)
    with pytest.raises(ValueError, match="key_timeline"):
        _gather(ctx, dev, case, [row[:5] for row in ROWS], None, key_timeline=_tabs(dev, tabs))


@pytest.mark.parametrize("what", ["job -1", "job J", "empty range", "range past P", "negative offset"])
def test_a_bad_job_or_breakpoint_range_is_zeros_and_no_fault(ctx, dev, lib_path, what):
    """A bad table entry is valid input: the row is zeros, its neighbours are formed, the error word names the call once."""
    case = _gather_case(dev)
    off, frame, semi, fac = KC.tables(KEY_JOBS)
    off, bad_row = off.copy(), list(ROWS[0])
    if what == "job -1":
        bad_row[5] = -1
    elif what == "job J":
        bad_row[5] = 4
    elif what == "empty range":
        off[1] = off[2]                       # job 1 owns nothing (job 0 takes its points: still inside [0, P))
    elif what == "range past P":
        bad_row[5], off[4] = 3, 11            # job 3's range ends behind the P = 10 breakpoints
    else:
        bad_row[5], off[0] = 0, -1            # job 0's range starts before the table
    torch.cuda.synchronize()
    ctx.poll_error()
    rows = [ROWS[5], tuple(bad_row), ROWS[6]]                                     # (job 2's range is the same in every case)
    wav, f0_rows, vol_rows = _gather(ctx, dev, case, rows, None, key_timeline=_tabs(dev, (off, frame, semi, fac)))
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="ddsp_pieces_gather"):
        ctx.poll_error()
    ctx.poll_error()                                                              # reported once
    assert not wav[1].any() and not f0_rows[1].any() and not vol_rows[1].any()
    want, _, bad = KC.gather_f0(case[1], N_FRAMES, rows, (off, frame, semi, fac), N_MAX)
    assert bad.tolist() == [False, True, False]
    assert np.array_equal(f0_rows.cpu().numpy()[[0, 2]], want[[0, 2]])            # (both neighbours are stored-factor rows)
    assert torch.isfinite(wav).all() and torch.isfinite(f0_rows).all() and torch.isfinite(vol_rows).all()


# ---- 2. jobs end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(dev, lib_path):
    return [bank_model("CombSub", 2, 43, dev), bank_model("Sins", 2, 44, dev)]


def _noise(dev, slices, jobs, seed=913):
    import infer_offline
    pieces = infer_offline.piece_table(slices, float(HOP))
    rng = np.random.Generator(np.random.PCG64(seed))
    return [[torch.from_numpy(rng.random(row[2] * HOP, dtype=np.float32)).to(dev) for row in pieces if row[0] == job[0]] for job in jobs]


def _eager_job(models, dev, files, job, points, noise, **kw):
    """Job `job` rendered slice by slice from f0 shifted on the host by the STATEMENT's factors (`points`: its breakpoints in file
    frames) -> the job's waveform, as `render_device` stitches it."""
    import infer_offline
    k, m, spk, _ = job
    segments, f0, volume = infer_offline.file_features(files, k)                  # (analysed with keys = 0: f0 as extracted)
    n = f0.shape[1]
    times, semi = [p[0] for p in points], np.array([p[1] for p in points], dtype=np.float32)
    factor, _ = KC.factors(times, semi, [KC.stored_factor(p[1]) for p in points], np.arange(n, dtype=np.float64))
    shifted = f0 * torch.from_numpy(factor).to(dev)[None, :, None]                # one rounded fp32 product per frame
    spk_id = torch.tensor([[spk]], dtype=torch.int64, device=dev)
    return infer_offline.render_device(models[m], _args(), segments, shifted, volume, spk_id, noise=noise, **kw)[0]


def test_jobs_with_a_moving_key_end_to_end(dev, lib_path, models, encoder, extractor):  # noqa: F811
    """Two files (1.3 s in two slices - the second starts at file frame 77 -, 0.7 s), three jobs, every row a group of its own,
    injected noise.  Job 0: a slope over file 0 whose middle breakpoint lies inside the second slice; job 1: a numeric key on the
    other model; job 2: a one-point timeline."""
    import infer_offline
    from infer_offline import KeyTimeline
    audios, slices = _files()
    tl = KeyTimeline([(0.1, -2.0), (1.0, 3.0), (1.25, 1.0)])
    jobs = [(0, 0, 1, tl), (1, 1, 2, 3.0), (0, 1, 1, KeyTimeline([(0, 3.0)]))]
    numeric = [(0, 0, 1, 0.0), (1, 1, 2, 3.0), (0, 1, 1, 3.0)]
    noise = _noise(dev, slices, jobs)
    run = lambda jj: infer_offline.convert_many_device(None, _args(), audios, SR, encoder, extractor, slices=slices, jobs=jj,  # noqa: E731
                                                       models=models, batch_frames=1, noise=noise)
    got, spans, sr_o = run(jobs)
    ref, ref_spans, _ = run(numeric)
    torch.cuda.synchronize()
    infer_offline.hipddsp.context_for(dev).poll_error()
    assert spans == ref_spans and sr_o == SR
    span = lambda x, j: x[spans[j][0]:spans[j][0] + spans[j][1]]  # noqa: E731
    # a numeric key beside a timeline, and KeyTimeline([(0, 3.0)]) against the key 3.0: the same bits
    assert torch.equal(span(got, 1), span(ref, 1)) and torch.equal(span(got, 2), span(ref, 2))
    assert float(span(ref, 2).abs().max()) > 1e-3 and rms((span(got, 0) - span(ref, 0)).cpu()) > 1e-3    # the moving key is heard
    # the slope against the per-slice eager forward on f0 times the statement's factors
    files = infer_offline.analyse_many(_args(), audios, SR, slices, encoder, extractor, 0, None)
    at, keys = tl.frames(SR, HOP)
    assert at == [9, 86, 108] and [row[1] for row in files["pieces"] if row[0] == 0] == [0, 77]
    want = _eager_job(models, dev, files, jobs[0], list(zip(at, keys)), noise[0])
    e = rms((span(got, 0) - want).cpu())
    print(f"the slope job against the eager render on the statement's f0: rms {e:.3e}")
    assert want.numel() == spans[0][1] and e < GATE and float(want.abs().max()) > 1e-3
    # a call without timelines equals itself with the tables forced: numeric keys through the new symbol
    plain, plain_spans, _ = infer_offline.render_jobs_device(models, _args(), files, numeric, batch_frames=300, noise=noise)
    forced, forced_spans, _ = infer_offline.render_jobs_device(models, _args(), files, numeric, batch_frames=300, noise=noise,
                                                               key_tables_always=True)
    torch.cuda.synchronize()
    infer_offline.hipddsp.context_for(dev).poll_error()
    assert plain_spans == forced_spans and torch.equal(plain, forced) and float(plain.abs().max()) > 1e-3


def test_jobs_with_a_moving_key_and_the_enhancer(dev, lib_path, models, encoder, extractor, tmp_path):  # noqa: F811
    """The enhancer's f0 is gathered again (`_enhance_many`): with a timeline it is the same moving f0.  The small generator of
    tests/test_gpu_many.py; every job against `render_device` with the enhancer on the eager f0, rms <= 1e-4 as there."""
    import infer_offline
    from infer_offline import KeyTimeline
    enh = _fixed_enhancer(tmp_path, dev)
    audios, slices = _files()
    tl = KeyTimeline([(0.1, 0.0), (0.6, 4.0)])
    jobs = [(1, 0, 1, tl), (0, 0, 2, -2.0)]
    noise = _noise(dev, slices, jobs, seed=914)
    files = infer_offline.analyse_many(_args(), audios, SR, slices, encoder, extractor, 0, None)
    kw = dict(enhancer=enh, enhancer_adaptive_key=2)
    got, spans, sr_o = infer_offline.render_jobs_device(models, _args(), files, jobs, batch_frames=1, noise=noise, **kw)
    torch.cuda.synchronize()
    infer_offline.hipddsp.context_for(dev).poll_error()
    at, keys = tl.frames(SR, HOP)
    for j, points in enumerate((list(zip(at, keys)), [(0, -2.0)])):
        want = _eager_job(models, dev, files, jobs[j], points, noise[j], **kw)
        base, total = spans[j]
        e = rms((got[base:base + total] - want).cpu())
        print(f"enhancer, job {j}: {total} samples, rms {e:.3e}")
        assert total == want.numel() and e <= 1e-4 and float(want.abs().max()) > 1e-3, (j, e)


# ---- 3. the bank kernel ---------------------------------------------------------------------------------------------------------
def _assert_factors(got, want, stored, what):
    d = KC.ulps(got, want)
    print(f"{what}: {int(stored.sum())} of {stored.size} frames owed exactly, largest distance {d.max():.2f} ulp")
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got[stored], want[stored]) and d.max() <= 1, what


def test_bank_kernel_matches_the_statement(ctx, dev, lib_path):
    """S = 3, W = 2, rows = [2, -1]; a 0.2 s block at 48 kHz for a 44.1 kHz model with 512-sample frames: hop 557.28.., fractional.
    Slot 2 ramps over both calls; slots 0 and 1 are not named."""
    import realtime
    z = realtime.bank_sizes(48000, 0.2, 0.04, 4, 512, 44100)
    block, n_in, Fr, hop = z["block"], z["n_in"], z["frames"], z["hop_size"]
    assert block == 9600 and hop != int(hop)
    S, P = 3, 4
    s = dict(clock=np.array([11, 22, 3000], dtype=np.int64), key_n=np.array([2, 0, 3], dtype=np.int32),
             key_t=np.zeros((S, P), dtype=np.int64), key_semi=np.zeros((S, P), dtype=np.float32),
             key_fac=np.ones((S, P), dtype=np.float32), pitch=np.array([1.5, 0.75, 1.25], dtype=np.float32))
    first = 3000 + block - n_in                                    # tau of frame 0 in call 1
    times = [first + 3 * 557, first + n_in + block + 5000, first + 10 * block]   # frame 3 of call 1 is the first behind the first
    keys = [-1.0, 2.0, 0.5]                                                       # point; the second lies behind both windows
    s["key_t"][2, :3], s["key_semi"][2, :3], s["key_fac"][2, :3] = times, keys, [KC.stored_factor(k) for k in keys]
    s["key_t"][0, :2], s["key_semi"][0, :2], s["key_fac"][0, :2] = [5, 50000], [1, 2], [KC.stored_factor(1), KC.stored_factor(2)]
    t = {k: torch.from_numpy(v.copy()).to(dev) for k, v in s.items()}
    rows = [2, -1]
    out = torch.full((2, Fr), float("nan"), device=dev)
    seen = []
    for call in range(2):
        got = ctx.bank_key_glide_(_i32(dev, rows), t["clock"], t["key_n"], t["key_t"], t["key_semi"], t["key_fac"], t["pitch"], out,
                                  n_in, block, hop)
        torch.cuda.synchronize()
        ctx.poll_error()                                           # a padding row is no error
        assert got is out
        want, stored, s["clock"] = KC.bank_pitch_frames(rows, 2, **s, Fr=Fr, n_in=n_in, block=block, hop=hop)
        _assert_factors(out.cpu().numpy(), want, stored, f"call {call + 1}")
        assert np.array_equal(out[1].cpu().numpy(), np.ones(Fr, dtype=np.float32)) and not stored[0].all()
        seen.append(out[0].cpu().numpy().copy())
    # the second call continues the slope: it saw the window one block later
    assert np.array_equal(seen[0][:3], np.full(3, KC.stored_factor(-1.0))) and (np.diff(seen[0][3:]) > 0).all()
    assert (np.diff(seen[1]) > 0).all() and (seen[1] > seen[0]).all() and seen[1].max() < KC.stored_factor(2.0)
    assert t["clock"].tolist() == [11, 22, 3000 + 2 * block] == s["clock"].tolist()
    for name in ("key_n", "key_t", "key_semi", "key_fac", "pitch"):                # nothing else was written; slots 0, 1 untouched
        assert np.array_equal(t[name].cpu().numpy(), s[name]), name
    # rows = None: row r is slot r; a slot with key_n = 0 gets pitch[s]
    out3 = torch.full((S, Fr), float("nan"), device=dev)
    ctx.bank_key_glide_(None, t["clock"], t["key_n"], t["key_t"], t["key_semi"], t["key_fac"], t["pitch"], out3, n_in, block, hop)
    torch.cuda.synchronize()
    want, stored, clock = KC.bank_pitch_frames(None, S, **s, Fr=Fr, n_in=n_in, block=block, hop=hop)
    _assert_factors(out3.cpu().numpy(), want, stored, "rows = None")
    assert np.array_equal(out3[1].cpu().numpy(), np.full(Fr, np.float32(0.75))) and t["clock"].tolist() == clock.tolist()
    for bad in (dict(n_in=n_in, block=0, hop=hop), dict(n_in=n_in, block=block, hop=0.0)):
        with pytest.raises(ValueError):
            ctx.bank_key_glide_(None, t["clock"], t["key_n"], t["key_t"], t["key_semi"], t["key_fac"], t["pitch"], out3, **bad)
    with pytest.raises(ValueError):
        ctx.bank_key_glide_(None, t["clock"].int(), t["key_n"], t["key_t"], t["key_semi"], t["key_fac"], t["pitch"], out3, n_in, block, hop)


# ---- 4. the bank end to end -----------------------------------------------------------------------------------------------------
S, K, P_MAX = 3, 3, 4
BLOCK_TIME, XFADE_TIME, BUFFER_NUM, THR = 0.1, 0.04, 4, -45.0       # the geometry of tests/test_gpu_bank_glide.py


@pytest.fixture(scope="module")
def model(dev, lib_path):
    return synthetic.build_model("CombSub", seed=43, device=dev)[0]


def _bank(model, dev, **kw):
    import realtime
    return realtime.StreamBank(model, S, SR, BLOCK_TIME, XFADE_TIME, dev, buffer_num=BUFFER_NUM, threshold_db=THR, max_mix=K, **kw)


def _inputs(k, bank, dev):
    rng = np.random.Generator(np.random.PCG64(700 + k))
    t = (np.arange(bank.block) + k * bank.block) / SR
    blocks = np.stack([0.2 * np.sin(2 * np.pi * f * t) + 0.01 * rng.standard_normal(bank.block) for f in (147.0, 220.0, 330.0)])
    z = synthetic.make_inputs(8100 + k, S, bank.frames)
    return {"blocks": torch.from_numpy(blocks.astype(np.float32)).to(dev), "units": z["units"].to(dev), "f0": z["f0"].to(dev),
            "noise": z["noise"].to(dev)}


def _push(bank, x, active=None):
    row = (lambda name: x[name]) if active is None else (lambda name: x[name][list(active)].contiguous())
    return bank.push_block(row("blocks"), row("units"), row("f0"), noise=row("noise"), **({} if active is None else {"active": active}))


def _key_state(bank):
    return {name: getattr(bank, "key_" + name).cpu().numpy() for name in ("clock", "n", "t", "semi", "fac")}


def _statement(bank, z, rows=None, W=S):
    """The statement on a bank's state `z` (`_key_state`) -> (pitch_frames, stored); advances z['clock']."""
    want, stored, z["clock"] = KC.bank_pitch_frames(rows, W, z["clock"], z["n"], z["t"], z["semi"], z["fac"], bank.pitch.cpu().numpy(),
                                                    Fr=bank.frames, n_in=bank.n_in, block=bank.block, hop=bank.hop_size)
    return want, stored


def test_unused_and_constant_timelines_emit_todays_bits(dev, model):
    """A bank with `pitch_breakpoints` and no timeline set, and one with a constant timeline at k semitones, against the bank
    built without the option under `set_pitch`: emitted blocks and `last_signal` bit for bit."""
    from infer_offline import KeyTimeline
    plain, unused, const = _bank(model, dev), _bank(model, dev, pitch_breakpoints=P_MAX), _bank(model, dev, pitch_breakpoints=P_MAX)
    assert plain.graph_builds == unused.graph_builds == const.graph_builds == 1
    for s, k in enumerate((3.0, -2.0, 0.1)):
        plain.set_pitch(s, k)
        unused.set_pitch(s, k)
    const.set_pitch_timeline(0, KeyTimeline([(0.0, 3.0)]))
    const.set_pitch_timeline(1, KeyTimeline([(0.05, -2.0), (0.2, -2.0)]))
    const.set_pitch_timeline(2, KeyTimeline([(0.1, 0.1)]), at=0.3)
    for k in range(3):
        x = _inputs(k, plain, dev)
        a, b, c = _push(plain, x), _push(unused, x), _push(const, x)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c), k
        assert torch.equal(plain.last_signal, unused.last_signal) and torch.equal(plain.last_signal, const.last_signal), k
        assert torch.equal(plain.last_f0, const.last_f0) and float(a.abs().max()) > 0 and float(plain.last_signal.abs().max()) > 1e-3
        assert torch.equal(unused.last_pitch, unused.pitch[:, None].expand(S, unused.frames)) and plain.last_pitch is None
        assert torch.equal(const.last_pitch, unused.last_pitch)
    assert plain.graph_builds == unused.graph_builds == const.graph_builds == 1
    assert unused.key_clock.tolist() == [3 * unused.block] * S and not unused.key_n.any()
    assert const.key_clock.tolist() == [3 * const.block, 3 * const.block, 3 * const.block + int(round(0.3 * SR))]


def test_a_slope_against_the_statement_and_the_eager_chain(dev, model):
    """Five blocks; slot 1 ramps -2 -> +3 -> +1 semitones from 0.15 s to 0.35 s.  Per block `last_pitch` is the statement's,
    `last_f0` is the caller's f0 times it, and `last_signal` is the eager forward on the caller's f0 times the STATEMENT's
    factors, gated - bit for bit, as tests/test_gpu_bank_glide.py holds its eager comparison.  The graph and the eager bank agree
    bit for bit; `set_pitch_timeline`, `set_pitch` and `reset` capture nothing."""
    import hipddsp
    from infer_offline import KeyTimeline
    graph, eager = _bank(model, dev, pitch_breakpoints=P_MAX), _bank(model, dev, pitch_breakpoints=P_MAX, use_graph=False)
    assert graph.graph_builds == 1 and eager.graph_builds == 0
    tl = KeyTimeline([(0.15, -2.0), (0.25, 3.0), (0.35, 1.0)])
    for bank in (graph, eager):
        bank.set_pitch(0, 2.0)
        bank.set_pitch_timeline(1, tl)
    assert graph.key_t[1].tolist() == [6615, 11025, 15435, 0] and graph.key_n.tolist() == [0, 3, 0]
    ctx = hipddsp.context_for(dev)
    z, moving = _key_state(graph), 0
    for k in range(5):
        x = _inputs(k, graph, dev)
        a, b = _push(graph, x), _push(eager, x)
        torch.cuda.synchronize()
        want, stored = _statement(graph, z)
        _assert_factors(graph.last_pitch.cpu().numpy(), want, stored, f"block {k + 1}")
        assert graph.key_clock.tolist() == z["clock"].tolist() == [(k + 1) * graph.block] * S
        moving += int((~stored[1]).sum())
        assert torch.equal(graph.last_pitch, eager.last_pitch) and torch.equal(a, b) and torch.equal(graph.last_signal, eager.last_signal), k
        f0 = x["f0"] * torch.from_numpy(want).to(dev)[:, :, None]
        assert torch.equal(graph.last_f0, f0), k
        with torch.no_grad():
            sig = model(graph.last_units, f0, graph.last_volume, None, spk_mix_rows=(graph.spk_ids, graph.spk_w), noise=x["noise"])[0]
        ctx.volume_gate_(sig, graph.last_volume, THR, 512)
        torch.cuda.synchronize()
        assert torch.equal(graph.last_signal, sig), (k, float((graph.last_signal - sig).abs().max()))
        assert float(sig[1].abs().max()) > 1e-3
    assert moving > 20 and len(set(graph.last_pitch[1].tolist())) > 5
    assert graph.last_pitch[1, -1].item() == KC.stored_factor(1.0) and graph.last_pitch[0, 0].item() == KC.stored_factor(2.0)
    # ending and restarting a timeline: device rows only
    graph.set_pitch(1, 1.0)
    graph.reset(1)
    _push(graph, _inputs(5, graph, dev))
    torch.cuda.synchronize()
    assert torch.equal(graph.last_pitch[1], torch.full((graph.frames,), float(KC.stored_factor(1.0)), device=dev))
    assert graph.key_n.tolist() == [0, 0, 0] and graph.key_clock.tolist() == [6 * graph.block, graph.block, 6 * graph.block]
    assert graph.graph_builds == 1 and eager.graph_builds == 0


def test_a_paused_slots_key_stands_still_and_resumes(dev, model):
    """`active_widths=(1, 2)`; slot 2's key glides and is named in calls 1 and 4 only.  Through calls 2 and 3 its rows of the five
    tensors stay bit for bit, and call 4 gives it the factors of a bank in which it saw two calls."""
    from infer_offline import KeyTimeline
    tl = KeyTimeline([(0.0, 0.0), (0.3, 4.0)])
    bank, other = (_bank(model, dev, pitch_breakpoints=P_MAX, active_widths=(1, 2)) for _ in range(2))
    assert bank.graph_builds == other.graph_builds == 4
    for b in (bank, other):
        b.set_pitch_timeline(2, tl)
        b.set_pitch_timeline(0, KeyTimeline([(0.05, 1.0), (0.2, 2.0)]))
    kept = lambda: [t.clone() for t in (bank.key_clock[2], bank.key_n, bank.key_t, bank.key_semi, bank.key_fac, bank.pitch, bank.windows[2])]  # noqa: E731
    calls = [[0, 2], [0, 1], [1], [1, 2]]
    z = _key_state(bank)
    for n, active in enumerate(calls):
        _push(bank, _inputs(n, bank, dev), active=active)
        torch.cuda.synchronize()
        want, stored = _statement(bank, z, rows=active, W=len(active))
        _assert_factors(bank.last_pitch.cpu().numpy(), want, stored, f"call {n + 1}")
        assert bank.last_pitch.shape == (len(active), bank.frames) and bank.last_active == tuple(active)
        if n == 0:
            after_first = kept()
            assert int(bank.key_clock[2]) == bank.block
        elif n < 3:
            for got, ref in zip(kept(), after_first):
                assert torch.equal(got, ref), n
    assert bank.key_clock.tolist() == [2 * bank.block, 3 * bank.block, 2 * bank.block] == z["clock"].tolist()
    _push(other, _inputs(0, other, dev), active=[0, 2])
    _push(other, _inputs(3, other, dev), active=[1, 2])
    torch.cuda.synchronize()
    assert torch.equal(bank.last_pitch[1], other.last_pitch[1]) and len(set(bank.last_pitch[1].tolist())) > 5
    assert torch.equal(bank.last_pitch[0], torch.ones(bank.frames, device=dev)) and bank.graph_builds == 4


def test_a_slope_on_a_slot_of_each_model(dev, lib_path):
    """`models=[m0, m1]` (CombSub, Sins), where the speaker glide is refused: the pitch is applied in the shared analysis, in front
    of the per-model gathers.  A slope on a slot of each model; the f0 both models render is the caller's times the statement."""
    from infer_offline import KeyTimeline
    m0, m1 = bank_model("CombSub", 1, 43, dev), bank_model("Sins", 3, 44, dev)
    bank = _bank(None, dev, models=[m0, m1], pitch_breakpoints=P_MAX)
    plain = _bank(None, dev, models=[m0, m1])
    for b in (bank, plain):
        b.set_model(1, 1, spk_id=2)
        b.set_model(2, 1, spk_id=3)
    builds = bank.graph_builds
    assert builds == plain.graph_builds
    bank.set_pitch_timeline(0, KeyTimeline([(0.0, 0.0), (0.3, 5.0)]))
    bank.set_pitch_timeline(2, KeyTimeline([(0.05, 2.0), (0.25, -3.0)]))
    z, moving = _key_state(bank), 0
    for k in range(3):
        x = _inputs(k, bank, dev)
        a, b = _push(bank, x), _push(plain, x)
        torch.cuda.synchronize()
        want, stored = _statement(bank, z)
        _assert_factors(bank.last_pitch.cpu().numpy(), want, stored, f"block {k + 1}")
        assert torch.equal(bank.last_f0, x["f0"] * torch.from_numpy(want).to(dev)[:, :, None]), k
        moving += int((~stored[[0, 2]]).sum())
        # slot 1 has no timeline: the bits of the bank without the option; the gliding slots differ from it
        assert torch.equal(bank.last_signal[1], plain.last_signal[1]) and torch.equal(a[1], b[1]), k
        assert rms((bank.last_signal[0] - plain.last_signal[0]).cpu()) > 1e-4 or k == 0
    assert moving > 20 and rms((bank.last_signal[2] - plain.last_signal[2]).cpu()) > 1e-4
    assert bank.graph_builds == builds
