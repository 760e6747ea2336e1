"""Offline conversion of JOBS on the device: `convert_many_device(jobs=, models=)` - a job is a file, a model, a speaker or mix
and a key - against `convert_many_device` of every job's file alone with that model, speaker and key; one analysis whatever
the number of jobs; the six-column gather (`ddsp_pieces_gather_jobs`) and its bounds; an empty job list; `main.run --jobs`.

Three synthesisers of `synthetic.MODEL_CFG` widths with two speakers each (CombSub, Sins, CombSubFast), two synthetic files at
the model rate - 1.3 s with 0.4 s of silence inside it, given as two slices, and 0.7 s - the 'ac' extractor (no weights, no
dither) and a random-weight HubertSoft.  The units are encoded a slice per group on both sides, so the features of a job and of
its solo call are the same bits and only the grouping of the render differs.

Bounds are quoted: where the solo call makes the very launches of the jobs call (a slice per group on both sides, the same
speaker form) the spans are equal bit for bit; a row of a larger ragged group against the row alone is held to rms < 1e-4
(`GATE` of tests/test_gpu_ragged.py, through tests/test_gpu_many.py, which holds grouped against solo renders to it)."""
import numpy as np
import pytest
import torch

import synthetic
from conftest import rms
from test_bank_models_host import bank_model
from test_gpu_many import GATE, _voiced
from test_gpu_many import encoder  # noqa: F401  (the module-scoped random-weight HubertSoft fixture)

pytestmark = pytest.mark.gpu
SR, HOP = synthetic.SR, synthetic.HOP
MIX = {1: 0.25, 2: 0.75}
# file 0 to all three models, at keys 0 and +3, by id and by a mix; file 1 to two of them
JOBS = [(0, 0, 1, 0), (0, 1, MIX, 3), (0, 2, 2, 3), (1, 0, 2, 3), (1, 2, 1, 0)]


@pytest.fixture(scope="module")
def models(dev, lib_path):
    return [bank_model("CombSub", 2, 43, dev), bank_model("Sins", 2, 44, dev), bank_model("CombSubFast", 2, 45, dev)]


@pytest.fixture(scope="module")
def extractor(dev, lib_path):
    from ddsp.vocoder import F0_Extractor
    return F0_Extractor("ac", SR, HOP, 65.0, 800.0, device=dev)


def _args():
    from ddsp.vocoder import DotDict
    return DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})


def _files():
    """File 0: 0.5 s voiced, 0.4 s of silence, 0.4 s voiced - its two slices leave the silence out; file 1: 0.7 s voiced."""
    a, b = _voiced(int(0.5 * SR), 150.0, 21), _voiced(int(0.4 * SR) + 7, 210.0, 22)
    first = np.concatenate([a, np.zeros(int(0.4 * SR), dtype=np.float32), b])
    second = _voiced(int(0.7 * SR) + 3, 120.0, 23)
    slices = [[(0, len(a)), (len(a) + int(0.4 * SR), len(first))], [(0, len(second))]]
    return [first, second], slices


def _noise(dev, slices):
    """One U[0,1) draw per job and slice of its file, (n_frames * HOP,) each."""
    import infer_offline
    pieces = infer_offline.piece_table(slices, float(HOP))
    rng = np.random.Generator(np.random.PCG64(909))
    return [[torch.from_numpy(rng.random(row[2] * HOP, dtype=np.float32)).to(dev) for row in pieces if row[0] == k]
            for k, _, _, _ in JOBS]


def _solo(models, dev, encoder, extractor, audios, slices, job, noise, batch_frames):
    """The job's file alone through today's call: one model, one speaker (an id, or the mix as a one-row table), one key."""
    import hipddsp
    import infer_offline
    k, m, spk, key = job
    kw = {"spk_ids": spk}
    if isinstance(spk, dict):
        ids, w = hipddsp.mix_rows([spk], len(spk), 2)
        kw = {"spk_ids": None, "spk_mix_rows": (ids.to(dev), w.to(dev))}
    out, spans, sr_o = infer_offline.convert_many_device(models[m], _args(), [audios[k]], SR, encoder, extractor, slices=[slices[k]],
                                                         keys=key, batch_frames=batch_frames, noise=[noise], **kw)
    assert spans == [(0, out.numel())] and sr_o == SR
    return out


@pytest.mark.parametrize("batch_frames", [1, 100000])
def test_jobs_equal_solo_calls(dev, lib_path, models, encoder, extractor, batch_frames):  # noqa: F811
    """batch_frames 1: every row is a group of its own, in the jobs call (model 0's three rows are three groups) and in the
    solo calls - the same launches, the same bits.  batch_frames 100000: one group per model against the solo calls' own
    groups - another grouping, held to the ragged gate."""
    import infer_offline
    audios, slices = _files()
    noise = _noise(dev, slices)
    table = infer_offline.job_table(infer_offline.piece_table(slices, float(HOP)), 2, JOBS, models)
    groups = infer_offline.job_groups(table, 3, batch_frames)
    assert [len(x) for x in table["starts_per_job"]] == [2, 2, 2, 1, 1]                    # file 0 has two slices
    if batch_frames == 1:
        assert [m for m, _ in groups] == [0, 0, 0, 1, 1, 2, 2, 2]
    else:
        assert [(m, len(g)) for m, g in groups] == [(0, 3), (1, 2), (2, 3)]
    got, spans, sr_o = infer_offline.convert_many_device(None, _args(), audios, SR, encoder, extractor, slices=slices, jobs=JOBS,
                                                         models=models, batch_frames=batch_frames, noise=noise)
    assert sr_o == SR and got.is_cuda and got.dtype == torch.float64 and len(spans) == len(JOBS)
    covered = torch.zeros(got.numel(), dtype=torch.bool, device=got.device)
    end = 0
    for j, ((base, total), job) in enumerate(zip(spans, JOBS)):
        want = _solo(models, dev, encoder, extractor, audios, slices, job, noise[j], batch_frames)
        assert base == end + (end & 1) and base % 2 == 0 and total == want.numel() and float(want.abs().max()) > 1e-3, j
        e = rms((got[base:base + total] - want).cpu())
        print(f"batch_frames {batch_frames} job {j} {job}: {total} samples from {base}, rms {e:.3e}")
        if batch_frames == 1:
            assert torch.equal(got[base:base + total], want), (j, e)
        assert e < GATE, (j, e)
        covered[base:base + total] = True
        end = base + total
    assert got.numel() == end and not got[~covered].any()
    # the jobs over file 0 differ (three models, two keys), and the silence between its slices is silent in each
    a, b, c = (got[base:base + total] for base, total in spans[:3])
    assert a.numel() == b.numel() == c.numel() and rms((a - b).cpu()) > 1e-3 and rms((b - c).cpu()) > 1e-3
    quiet = slice(int(0.6 * SR), int(0.8 * SR))
    assert not a[quiet].any() and not b[quiet].any() and not c[quiet].any()
    # the host-returning wrapper splits the same tensor
    waves, _ = infer_offline.convert_many(None, _args(), audios, SR, encoder, extractor, slices=slices, jobs=JOBS, models=models,
                                          batch_frames=batch_frames, noise=noise)
    assert [w.shape[0] for w in waves] == [t for _, t in spans] and np.array_equal(waves[3], got[spans[3][0]:].cpu().numpy()[:spans[3][1]])
    torch.cuda.synchronize()
    infer_offline.hipddsp.context_for(dev).poll_error()


def test_an_id_beside_a_mix_of_the_same_model(dev, lib_path, models, encoder, extractor):  # noqa: F811
    """A model with a mix among its jobs takes every one of its jobs as a mix row (a plain id is the row {id: 1.0}): the id
    job against its solo call by id - another speaker form of the control network, held to the gate."""
    import infer_offline
    audios, slices = _files()
    jobs = [(1, 1, 2, 0), (1, 1, MIX, 0), (1, 0, 1, 0)]
    noise = _noise(dev, slices)[3:4] * 3
    got, spans, _ = infer_offline.convert_many_device(models[0], _args(), audios, SR, encoder, extractor, slices=slices, jobs=jobs,
                                                      models=models, batch_frames=1, noise=noise)
    for j, job in enumerate(jobs):
        want = _solo(models, dev, encoder, extractor, audios, slices, job, noise[j], 1)
        base, total = spans[j]
        e = rms((got[base:base + total] - want).cpu())
        print(f"job {j} {job}: rms {e:.3e}")
        assert total == want.numel() and e < GATE, (j, e)
    assert rms((got[spans[0][0]:spans[0][0] + spans[0][1]] - got[spans[1][0]:spans[1][0] + spans[1][1]]).cpu()) > 1e-3


def test_one_analysis_whatever_the_number_of_jobs(dev, lib_path, models, encoder, extractor, monkeypatch):  # noqa: F811
    """Counting wrappers around the extractor, the encoder and the slicer (`slices=None`: the device slicer runs): J = 1 and
    J = 5 over the same two files make the same calls."""
    import infer_offline
    audios, _ = _files()
    calls = {"extract": 0, "encode": 0, "split": 0}

    def counted(name, fn):
        def wrapper(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapper
    monkeypatch.setattr(extractor, "extract", counted("extract", extractor.extract))
    monkeypatch.setattr(encoder, "encode", counted("encode", encoder.encode))
    monkeypatch.setattr(infer_offline.Slicer, "chunks", counted("split", infer_offline.Slicer.chunks))
    seen = []
    for jobs in (JOBS[:1], JOBS):
        for name in calls:
            calls[name] = 0
        out, spans, _ = infer_offline.convert_many_device(None, _args(), audios, SR, encoder, extractor, jobs=jobs, models=models,
                                                          batch_frames=300, noise_seed=7)
        assert len(spans) == len(jobs) and bool(torch.isfinite(out).all())
        seen.append(dict(calls))
    print(seen)
    assert seen[0] == seen[1] and seen[0]["extract"] == 1 and seen[0]["split"] == 1 and seen[0]["encode"] >= 2
    # the seed rule: the same call twice gives the same bits
    again, _, _ = infer_offline.convert_many_device(None, _args(), audios, SR, encoder, extractor, jobs=JOBS, models=models,
                                                    batch_frames=300, noise_seed=7)
    assert torch.equal(out, again)


def test_the_feature_is_there(lib_path):
    """On the parent commit `convert_many_device(..., jobs=...)` is a TypeError and `Context` has no `pcm16`."""
    import inspect

    import hipddsp
    import infer_offline
    assert "jobs" in inspect.signature(infer_offline.convert_many_device).parameters and hasattr(hipddsp.Context, "pcm16")


def test_tuples_and_records_render_the_same_bits(dev, lib_path, models, encoder, extractor):  # noqa: F811
    """Every control once - a speaker timeline, a key timeline, a numeric formant, a tune, an index, an envelope - and a plain
    job, over two short files of three and two slices and two models, in groups of one and two rows: the list as tuples and as
    `Job` records through `render_jobs_device`, the same seed.  The same launches on the same tables: equal bits, spans, rate."""
    import infer_offline
    from controls import EnvelopeMix, Job, KeyTimeline, PitchTune, SpeakerTimeline, UnitIndex, UnitIndexBank
    audios = [_voiced(22 * HOP + 100, 150.0, 31), _voiced(15 * HOP + 3, 210.0, 32)]
    slices = [[(0, 9 * HOP), (9 * HOP, 15 * HOP), (15 * HOP, 22 * HOP + 100)], [(0, 6 * HOP), (8 * HOP, 15 * HOP + 3)]]
    rng = np.random.default_rng(33)
    bank = UnitIndexBank([UnitIndex(rng.standard_normal((n, 256)).astype(np.float32)) for n in (5, 7)], device=dev, k=3)
    jobs = [(0, 0, SpeakerTimeline([(0.0, 1), (0.2, {1: 0.25, 2: 0.75})]), 0.0), (1, 1, 2, KeyTimeline([(0.0, 0.0), (0.15, 3.0)])),
            (0, 1, 1, 1.0, 2), (1, 0, MIX, 0.0, None, PitchTune.scale("A", "minor", retune=0.02)),
            (0, 0, 2, -2.0, None, None, (1, 0.5)), (1, 1, 1, 0.0, None, None, None, EnvelopeMix(0.25, 0.01, 4)), (1, 0, 1, 0.0)]
    records = [Job.of(j, job) for j, job in enumerate(jobs)]
    assert [len(job) for job in jobs] == [4, 4, 5, 6, 7, 8, 4] and all(isinstance(r, Job) for r in records)
    files = infer_offline.analyse_many(_args(), audios, SR, slices, encoder, extractor, 0, None)
    table = infer_offline.job_table(files["pieces"], 2, records, models[:2], len(bank))
    groups = infer_offline.job_groups(table, 2, 16)
    assert [row[2] for row in files["pieces"]] == [10, 7, 8, 7, 8]
    assert min(sum(1 for m, _ in groups if m == k) for k in (0, 1)) >= 2 and {len(g) for _, g in groups} == {1, 2}
    kw = dict(batch_frames=16, noise_seed=5, indices=bank, retrieve_k=3)
    got, spans, sr_o = infer_offline.render_jobs_device(models[:2], _args(), files, jobs, **kw)
    again, spans_again, sr_again = infer_offline.render_jobs_device(models[:2], _args(), files, records, **kw)
    torch.cuda.synchronize()
    infer_offline.hipddsp.context_for(dev).poll_error()
    assert spans == spans_again and len(spans) == len(jobs) and sr_o == sr_again == SR
    assert got.dtype == torch.float64 and bool(torch.isfinite(got).all()) and torch.equal(got, again)
    for j, (base, total) in enumerate(spans):
        assert total > 0 and float(got[base:base + total].abs().max()) > 1e-3, j


# ---- the six-column gather -------------------------------------------------------------------------------------------------

N_SAMPLES, N_FRAMES, JOB_KEYS = [700, 2051], [11, 33], [0, 3, -12, 5]
# (file, start_frame, n_frames, start_sample, n_samples, job): three jobs over file 1 - two over the same piece -, one over file 0
ROWS = [(1, 2, 17, 129, 1100, 0), (1, 2, 17, 129, 1100, 2), (0, 5, 6, 300, 400, 3), (1, 30, 3, 2050, 1, 1)]


def _gather_case(dev):
    rng = np.random.Generator(np.random.PCG64(616))
    nan = float("nan")
    audio, f0, volume = torch.full((2, 2051), nan), torch.full((2, 33), nan), torch.full((2, 33), nan)
    for k, (n, fr) in enumerate(zip(N_SAMPLES, N_FRAMES)):
        audio[k, :n] = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
        f0[k, :fr] = torch.from_numpy(rng.uniform(80.0, 700.0, fr).astype(np.float32))
        volume[k, :fr] = torch.from_numpy(rng.random(fr).astype(np.float32))
    factor = torch.tensor([2 ** (float(key) / 12) for key in JOB_KEYS], dtype=torch.float32)
    return audio.to(dev), f0.to(dev), volume.to(dev), factor.to(dev)


def _i32(dev, rows):
    return torch.tensor(rows, dtype=torch.int32).to(dev)


def test_rows_of_jobs_read_their_file_and_take_their_jobs_key(ctx, dev, lib_path):
    audio, f0, volume, factor = _gather_case(dev)
    ns_dev, nf_dev = _i32(dev, N_SAMPLES), _i32(dev, N_FRAMES)
    wav, f0_rows, vol_rows = ctx.pieces_gather(_i32(dev, ROWS), ns_dev, nf_dev, audio=audio, S_max=1101, f0=f0, volume=volume,
                                               key_factor=factor, N_max=19)
    for r, (k, sf, nf, ss, ns, j) in enumerate(ROWS):
        assert torch.equal(wav[r, :ns], audio[k, ss:ss + ns]) and not wav[r, ns:].any(), r
        assert torch.equal(f0_rows[r, :nf], f0[k, sf:sf + nf] * factor[j]) and not f0_rows[r, nf:].any(), r
        assert torch.equal(vol_rows[r, :nf], volume[k, sf:sf + nf]) and not vol_rows[r, nf:].any(), r
    assert torch.equal(wav[0], wav[1]) and torch.equal(vol_rows[0], vol_rows[1]) and not torch.equal(f0_rows[0], f0_rows[1])
    # a table of five columns over the same arrays keys by FILE, as before: (F,) key factors
    five = ctx.pieces_gather(_i32(dev, [row[:5] for row in ROWS]), ns_dev, nf_dev, f0=f0, key_factor=factor[:2].contiguous(), N_max=19)
    assert torch.equal(five[1][2, :6], f0[0, 5:11] * factor[0]) and torch.equal(five[1][0, :17], f0[1, 2:19] * factor[1])
    torch.cuda.synchronize()
    ctx.poll_error()


@pytest.mark.parametrize("bad", [(1, 2, 17, 129, 1100, 4), (1, 2, 17, 129, 1100, -1), (2, 2, 17, 129, 1100, 0),
                                 (0, 5, 7, 300, 400, 3), (1, 2, 17, 1000, 1100, 2), (1, 2, 17, 129, 1100, 2 ** 31 - 1)])
def test_a_row_outside_its_bounds_is_zeros_and_no_fault(ctx, dev, lib_path, bad):
    """A job outside [0, J) - just outside, negative, huge -, a file outside [0, F), frames and samples that leave the file: the
    row is written as zeros, its neighbours are formed, the error word names the call once."""
    audio, f0, volume, factor = _gather_case(dev)
    torch.cuda.synchronize()
    ctx.poll_error()
    rows = [ROWS[0], bad, ROWS[2]]
    wav, f0_rows, vol_rows = ctx.pieces_gather(_i32(dev, rows), _i32(dev, N_SAMPLES), _i32(dev, N_FRAMES), audio=audio, S_max=1100,
                                               f0=f0, volume=volume, key_factor=factor, N_max=17)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="ddsp_pieces_gather"):
        ctx.poll_error()
    ctx.poll_error()                                                              # reported once
    assert not wav[1].any() and not f0_rows[1].any() and not vol_rows[1].any()
    assert torch.equal(wav[0], audio[1, 129:1229]) and torch.equal(f0_rows[2, :6], f0[0, 5:11] * factor[3])
    assert torch.isfinite(wav).all() and torch.isfinite(f0_rows).all() and torch.isfinite(vol_rows).all()


def test_a_bad_entry_in_the_uploaded_table_and_an_empty_job_list(dev, lib_path, models, encoder, extractor):  # noqa: F811
    """The uploaded table of a call is kept in `files`; an entry overwritten there (a job far outside) reaches the kernel on the
    next render: that row is rendered from zeros, the call or the next poll raises, nothing faults, and a render from a
    fresh upload is what it was."""
    import infer_offline
    ctx = infer_offline.hipddsp.context_for(dev)
    audios, slices = _files()
    files = infer_offline.analyse_many(_args(), audios, SR, slices, encoder, extractor, 0, None)
    good, spans, _ = infer_offline.render_jobs_device(models, _args(), files, JOBS, batch_frames=100000, noise_seed=3)
    torch.cuda.synchronize()
    ctx.poll_error()
    assert files["table"].shape[1] == 6
    files["table"][1, 5] = 99
    raised = False
    try:
        infer_offline.render_jobs_device(models, _args(), files, JOBS, batch_frames=100000, noise_seed=3)
        torch.cuda.synchronize()
        ctx.poll_error()
    except ValueError as e:
        raised = "ddsp_pieces_gather" in str(e)
    assert raised
    torch.cuda.synchronize()
    ctx.poll_error()
    files.pop("table_rows")                                                       # a fresh upload
    again, spans_again, _ = infer_offline.render_jobs_device(models, _args(), files, JOBS, batch_frames=100000, noise_seed=3)
    assert spans_again == spans and torch.equal(again, good)
    out, none, sr_o = infer_offline.render_jobs_device(models, _args(), files, [], batch_frames=100000)
    assert out.numel() == 0 and out.dtype == torch.float64 and out.is_cuda and none == [] and sr_o == SR
    out, none, sr_o = infer_offline.convert_many_device(None, _args(), audios, SR, encoder, extractor, jobs=[], models=models)
    assert out.numel() == 0 and out.is_cuda and none == [] and sr_o == SR


# ---- the command line ------------------------------------------------------------------------------------------------------

def test_main_run_with_a_jobs_file(dev, lib_path, encoder, tmp_path, capsys):  # noqa: F811
    """`main.run --jobs`: two entries (another model by id at +3, the `-m` model by a mix) over a folder of two wavs -> four
    files `<name>_<suffix>.wav` holding `main.pcm16` of the jobs' spans of the returned tensor, file after file and entry after
    entry; the read-back is the int16 tensor."""
    import yaml
    from scipy.io import wavfile

    import main
    data = {"sampling_rate": SR, "block_size": HOP, "encoder": "hubertsoft", "encoder_ckpt": "unused", "encoder_sample_rate": 16000,
            "encoder_hop_size": 320, "encoder_out_channels": 256}
    for name, seed in (("CombSub", 8), ("Sins", 9)):
        model, _ = synthetic.build_model(name, seed=seed, device="cpu")
        (tmp_path / name).mkdir()
        with open(tmp_path / name / "config.yaml", "w") as fh:
            yaml.safe_dump({"data": data, "model": dict(synthetic.MODEL_CFG[name], c=False),
                            "enhancer": {"type": "nsf-hifigan", "ckpt": "unused"}}, fh)
        torch.save({"global_step": 0, "model": model.state_dict()}, tmp_path / name / "model_0.pt")
    audios = {"b.wav": _voiced(int(0.5 * SR), 130.0, 9), "a.wav": 4.0 * _voiced(int(0.4 * SR) + 5, 180.0, 10)}
    (tmp_path / "in").mkdir()
    for name, x in audios.items():
        wavfile.write(tmp_path / "in" / name, SR, x)
    with open(tmp_path / "jobs.yaml", "w") as fh:
        yaml.safe_dump([{"model": str(tmp_path / "Sins" / "model_0.pt"), "id": 2, "key": 3, "suffix": "sins"},
                        {"mix": {1: 0.5, 3: 0.5}, "suffix": "mix"}], fh)
    cmd = main.parse_args(["-m", str(tmp_path / "CombSub" / "model_0.pt"), "-i", str(tmp_path / "in"), "-o", str(tmp_path / "out"),
                           "-pe", "ac", "-e", "false", "--jobs", str(tmp_path / "jobs.yaml")])
    result, sr_o = main.run(cmd, units_encoder=encoder, device=dev)
    names = ["a_sins.wav", "a_mix.wav", "b_sins.wav", "b_mix.wav"]
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(names) and sr_o == SR
    host, base = result.cpu().numpy(), 0
    written, clipped = {}, []
    for name in names:
        total = (len(audios[name[0] + ".wav"]) // HOP + 1) * HOP                   # one slice: the whole file, in whole frames
        rate, written[name] = wavfile.read(tmp_path / "out" / name)
        assert rate == SR and written[name].dtype == np.int16 and int(np.abs(written[name]).max()) > 30, name
        assert np.array_equal(written[name], main.pcm16(host[base:base + total])), name
        r = np.rint(host[base:base + total] * 32768.0)
        if ((r < -32768) | (r > 32767)).any():
            clipped.append(name)
        base += total
    assert base == host.shape[0]
    assert not np.array_equal(written["a_sins.wav"], written["a_mix.wav"])
    # a warning line per output that clipped, and only for those
    lines = [x for x in capsys.readouterr().out.splitlines() if "[Warning]" in x]
    print(lines, clipped)
    assert len(lines) == len(clipped) and all(any(name in x for x in lines) for name in clipped)
