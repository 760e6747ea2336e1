"""The envelope mix, host side (no GPU): the numpy statement (tests/envelope_cases.py) against a second statement built from
other code - explicit `np.pad` and framing, `torch.nn.functional.interpolate` on an fp64 CPU tensor, RVC's three lines -,
`EnvelopeMix`, jobs of four to eight entries, the yaml forms of `main.py --jobs`, the bank's refusal with `models=`, the symbols."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import envelope_cases as EC
from conftest import ROOT
from test_bank_models_host import bank_model


# ---- the statement ----------------------------------------------------------------------------------------------------------------
def _rms_by_padding(x, hop, m):
    """librosa.feature.rms(y=x, frame_length=m * hop, hop_length=hop, center=True, pad_mode='constant') spelled out."""
    win = m * hop
    y = np.pad(np.asarray(x, dtype=np.float64), win // 2, mode="constant")
    frames = np.stack([y[i * hop:i * hop + win] for i in range(1 + (len(y) - win) // hop)])
    return np.sqrt(np.mean(frames ** 2, axis=1))


def _change_rms(src, hop1, out, hop2, m, rate):
    """RVC's `change_rms` behind its two librosa calls, on fp64 CPU tensors -> the gain."""
    rms1 = torch.from_numpy(_rms_by_padding(src, hop1, m))
    rms2 = torch.from_numpy(_rms_by_padding(out, hop2, m))
    rms1 = torch.nn.functional.interpolate(rms1.unsqueeze(0).unsqueeze(0), size=len(out), mode="linear", align_corners=False).squeeze()
    rms2 = torch.nn.functional.interpolate(rms2.unsqueeze(0).unsqueeze(0), size=len(out), mode="linear", align_corners=False).squeeze()
    rms2 = torch.max(rms2, torch.zeros_like(rms2) + 1e-6)
    return (torch.pow(rms1, torch.tensor(1 - rate)) * torch.pow(rms2, torch.tensor(rate - 1))).reshape(-1).numpy()


@pytest.mark.parametrize("hop,m", EC.RMS_SETTINGS + (EC.OFFLINE[:2], EC.LIVE[:2]))
def test_frame_rms_equals_explicit_padding(hop, m):
    lengths = EC.rms_lengths(hop) if hop < 100 else ([EC.OFFLINE[2]] if hop == EC.OFFLINE[0] else [EC.LIVE[2]])
    for n in lengths:
        x = EC.signal(n, seed=n)
        got, want = EC.frame_rms(x, hop, m), _rms_by_padding(x, hop, m)
        assert got.shape == want.shape == (1 + n // hop,) and np.allclose(got, want, rtol=1e-13, atol=0)


@pytest.mark.parametrize("rate", [0.0, 0.25])
@pytest.mark.parametrize("n1,hop1,n2,hop2,m", [(37, 4, 101, 11, 2), (3, 4, 7, 11, 2), (37, 5, 101, 7, 4), (8820, 441, 8192, 441, 4)])
def test_the_gain_equals_rvcs_lines(n1, hop1, n2, hop2, m, rate):
    """The kernel test's shapes (n1 / n2 not integral; N = 1) and the live size: 1e-13 relative on the gain."""
    src, out = EC.signal(n1, seed=1), EC.signal(n2, seed=2, dtype=np.float64)
    got, want = EC.gain(src, hop1, out, hop2, m, rate), _change_rms(src, hop1, out, hop2, m, rate)
    err = float(np.max(np.abs(got - want) / np.abs(want)))
    print(f"n1 {n1}, n2 {n2}, rate {rate}: the two statements differ by {err:.3e} relative")
    assert got.shape == (n2,) and err <= 1e-13


def test_the_cases_of_the_rule():
    src, out = EC.signal(37, seed=1), EC.signal(101, seed=2, dtype=np.float64)
    assert EC.same_bits(EC.mix(src, 4, out, 11, 2, 1.0), out) and EC.same_bits(EC.mix(src, 4, out, 11, 2, 1.5), out)
    assert EC.same_bits(EC.mix(src, 4, out, 11, 2, float("nan")), out)
    assert not EC.mix(np.zeros(37, dtype=np.float32), 4, out, 11, 2, 0.25).any()            # a silent source: the gain is exactly 0
    quiet = EC.signal(101, seed=3, scale=1e-9, dtype=np.float64)
    g = EC.gain(src, 4, quiet, 11, 2, 0.0)                                                  # the floor: e2 = 1e-6, g = e1 * 1e6
    assert np.allclose(g, EC.interpolate(EC.frame_rms(src, 4, 2), 101) * 1e6, rtol=1e-12)
    # rate 0 gives the output the source's envelope, up to what one gain per sample can do: the ratio of the two RMS stays near 1
    assert np.isfinite(EC.mix(src, 4, out, 11, 2, 0.0)).all()


# ---- EnvelopeMix and the jobs -------------------------------------------------------------------------------------------------------
def test_envelope_mix_fields():
    from infer_offline import EnvelopeMix
    e = EnvelopeMix(0.25)
    assert (e.rate, e.hop_seconds, e.frames) == (0.25, 0.5, 2) and e.setting(44100) == 22050 and e.setting(16000) == 8000
    assert EnvelopeMix(1, 0.01, 4).setting(44100) == 441 and EnvelopeMix(0).rate == 0.0
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "0.5", None, True):
        with pytest.raises(ValueError, match="rate"):
            EnvelopeMix(bad)
    for bad in (0, -1.0, float("nan"), float("inf"), "0.5", True):
        with pytest.raises(ValueError, match="hop_seconds"):
            EnvelopeMix(0.5, bad)
    for bad in (0, 1, 3, 10, 2.0, "2", True):
        with pytest.raises(ValueError, match="frames"):
            EnvelopeMix(0.5, 0.5, bad)
    with pytest.raises(ValueError, match="setting"):
        EnvelopeMix(0.5, 1e-6).setting(44100)                                               # a hop below one sample
    with pytest.raises(ValueError, match="setting"):
        e.setting(0)


def test_job_table_takes_four_to_eight_entries():
    import infer_offline
    from infer_offline import EnvelopeMix, PitchTune, envelope_tables, job_envelopes, job_table
    models = [bank_model("CombSub", 2, 43, "cpu")]
    pieces = [(0, 0, 10, 0, 5120), (1, 0, 8, 0, 4096)]
    tune, a, b = PitchTune(["A"]), EnvelopeMix(0.25), EnvelopeMix(0.0)
    jobs = [(0, 0, 1, 0.0), (1, 0, 2, 1.0, 2.0), (0, 0, 1, 0.0, None, tune), (1, 0, 1, 0.0, None, None, (1, 0.25)),
            (0, 0, 1, 0.0, None, None, None, a), (1, 0, 1, 0.0, 1.0, tune, (0, 0.5), b), (0, 0, 1, 0.0, None, None, None)]
    table = job_table(pieces, 2, jobs, models, 2)
    assert table == job_table(pieces, 2, [j[:6] for j in jobs], models)                     # its existing keys, and no new one
    assert set(table) == {"rows", "piece_of_row", "model_of_job", "speakers", "key_factor", "starts_per_job", "keys"}
    assert job_envelopes(jobs) == [None, None, None, None, a, b, None]
    assert infer_offline.job_indices(jobs)[5] == (0, 0.5) and infer_offline.job_tunes(jobs)[5] is tune
    rate, hop_seconds, frames = envelope_tables(job_envelopes(jobs))
    assert rate.dtype == torch.float64 and rate.tolist() == [1, 1, 1, 1, 0.25, 0, 1] and (hop_seconds, frames) == (0.5, 2)
    rate, hop_seconds, frames = envelope_tables([None, None])
    assert rate.tolist() == [1, 1] and hop_seconds is None and frames is None
    for bad in (0.5, "0.5", (0.5,), {"rate": 0.5}):
        with pytest.raises(ValueError, match="job 1: envelope"):
            job_table(pieces, 2, [jobs[0], (0, 0, 1, 0.0, None, None, None, bad)], models)
    for bad in ((0, 0, 1, 0.0, None, None, None, None, None), (0, 0, 1, 0.0, None, None, None, a, None),
                (0, 0, 1, 0.0, None, None, None, None)):                                  # (a job without one is the shorter tuple)
        with pytest.raises(ValueError, match="job 0 must be"):
            job_table(pieces, 2, [bad], models)
    off = EnvelopeMix(1.0)                                                                  # switched off, and still a job that has it
    assert envelope_tables(job_envelopes([(0, 0, 1, 0.0, None, None, None, off)]))[0].tolist() == [1.0]
    for other in (EnvelopeMix(0.5, 0.25), EnvelopeMix(0.5, 0.5, 4)):                         # mixed hop or window: refused
        with pytest.raises(ValueError, match="share hop_seconds and frames"):
            job_table(pieces, 2, [jobs[4], (0, 0, 1, 0.0, None, None, None, other)], models)
        with pytest.raises(ValueError, match="share hop_seconds and frames"):
            envelope_tables([a, None, other])


def test_mixed_settings_are_refused_before_anything_is_launched():
    """`convert_many_device` checks the tables in front of the analysis: no encoder, extractor or device is touched."""
    from ddsp.vocoder import DotDict
    from infer_offline import EnvelopeMix, convert_many_device
    models = [bank_model("CombSub", 2, 43, "cpu")]
    args = DotDict({"data": {"block_size": 512, "sampling_rate": 44100}})
    jobs = [(0, 0, 1, 0.0, None, None, None, EnvelopeMix(0.5)), (0, 0, 1, 0.0, None, None, None, EnvelopeMix(0.5, 0.1))]
    with pytest.raises(ValueError, match="share hop_seconds and frames"):
        convert_many_device(None, args, [np.zeros(4096, dtype=np.float32)], 44100, None, None, jobs=jobs, models=models)


def test_main_takes_an_envelope():
    import main
    from infer_offline import EnvelopeMix, job_table
    base = ["-m", "m.pt", "-i", "in.wav", "-o", "out.wav"]
    plain = main.parse_args(base)
    assert not hasattr(plain, "rms_mix_rate") and main._cmd_envelope(plain) is None
    cmd = main.parse_args(base + ["--rms_mix_rate", "0.25"])
    e = main._cmd_envelope(cmd)
    assert isinstance(e, EnvelopeMix) and (e.rate, e.hop_seconds, e.frames) == (0.25, 0.5, 2)
    with pytest.raises(ValueError, match="--rms_mix_rate"):
        main._cmd_envelope(main.parse_args(base + ["--rms_mix_rate", "1.5"]))
    # the yaml forms
    assert main._job_entry(0, {"id": 2, "key": 3, "envelope": 0.5, "suffix": "a"}) == (2, 3.0)
    assert main._job_envelope(0, {"suffix": "a"}) is None and main._job_envelope(0, {"suffix": "a"}, e) is e
    got = main._job_envelope(0, {"envelope": 0.5})
    assert (got.rate, got.hop_seconds, got.frames) == (0.5, 0.5, 2)
    got = main._job_envelope(0, {"envelope": {"rate": 0, "hop_ms": 10, "frames": 4}}, e)
    assert (got.rate, got.hop_seconds, got.frames) == (0.0, 0.01, 4)
    for bad in ("0.5", [0.5], True, {"hop_ms": 10}, {"rate": 0.5, "hop": 10}, {"rate": 1.5}, {"rate": 0.5, "frames": 3}, 2):
        with pytest.raises(ValueError, match="entry 3"):
            main._job_envelope(3, {"envelope": bad})
    # the job as job_table takes it: a record per file, with None for every control the voice does not carry
    Job = main.Job
    bare, indexed, mixed = Job(None, 1, 2, 3.0), Job(None, 1, 2, 3.0, index=(1, 0.5)), Job(None, 1, 2, 3.0, envelope=e)
    assert main._file_jobs(2, [bare, mixed]) == [Job(0, 1, 2, 3.0), Job(0, 1, 2, 3.0, None, None, None, e),
                                                  Job(1, 1, 2, 3.0), Job(1, 1, 2, 3.0, None, None, None, e)]
    (job,) = main._file_jobs(1, [bare])
    assert (job.file, job.model, job.spk, job.key) == (0, 1, 2, 3.0) and (job.formant, job.tune, job.index, job.envelope) == (None,) * 4
    (job,) = main._file_jobs(1, [indexed])
    assert (job.formant, job.tune, job.index, job.envelope) == (None, None, (1, 0.5), None)
    (job,) = main._file_jobs(1, [mixed])
    assert (job.formant, job.tune, job.index) == (None, None, None) and job.envelope is e
    job_table([(0, 0, 10, 0, 5120)], 1, main._file_jobs(1, [Job(None, 0, 1, 0.0, envelope=e)]), [bank_model("CombSub", 2, 43, "cpu")])


# ---- the bank, the entry points and the symbols --------------------------------------------------------------------------------------
def test_the_bank_refuses_before_the_device():
    """Every refusal of the constructor comes before anything is allocated: no device is needed."""
    import realtime
    m0, m1 = bank_model("CombSub", 2, 43, "cpu"), bank_model("Sins", 2, 44, "cpu")
    kw = dict(units_encoder=object(), f0_extractor="ac")
    with pytest.raises(ValueError, match="envelope=True with models="):
        realtime.StreamBank(None, 2, 44100, 0.1, 0.04, "cpu", models=[m0, m1], envelope=True, **kw)
    with pytest.raises(ValueError, match="envelope must be True or False"):
        realtime.StreamBank(m0, 2, 44100, 0.1, 0.04, "cpu", envelope=1, **kw)
    with pytest.raises(ValueError, match="needs units_encoder= and f0_extractor="):
        realtime.StreamBank(m0, 2, 44100, 0.1, 0.04, "cpu", envelope=True)
    for bad in (dict(envelope_frames=3), dict(envelope_hop_seconds=0), dict(envelope_hop_seconds=1e-7)):
        with pytest.raises(ValueError, match="StreamBank: EnvelopeMix"):
            realtime.StreamBank(m0, 2, 44100, 0.1, 0.04, "cpu", envelope=True, **kw, **bad)


def test_the_entry_points_take_the_control_as_arguments_with_defaults():
    import graphed
    import infer_offline
    import realtime
    # (in front of `tune` and `retrieve`, whose places at the end tests/test_retrieval_host.py pins; it is passed by keyword)
    assert list(inspect.signature(graphed.block_chain).parameters)[-3:] == ["envelope", "tune", "retrieve"]
    assert list(inspect.signature(graphed.GraphedBlock.__init__).parameters)[-3:] == ["envelope", "tune", "retrieve"]
    assert inspect.signature(graphed.block_chain).parameters["envelope"].default is None
    p = inspect.signature(realtime.StreamBank.__init__).parameters
    assert list(p)[-3:] == ["envelope", "envelope_hop_seconds", "envelope_frames"]
    assert (p["envelope"].default, p["envelope_hop_seconds"].default, p["envelope_frames"].default) == (False, 0.01, 4)
    assert "envelope" not in inspect.signature(infer_offline.render_many_device).parameters   # a job list serves
    assert hasattr(realtime.StreamBank, "set_envelope") and not hasattr(realtime.StreamRenderer, "set_envelope")
    with pytest.raises(ValueError, match="needs the model"):
        graphed.block_chain(_Ctx(), None, _Encoder(), _Extractor(), torch.zeros(2, 64), torch.zeros(2, 8), 16000, 8, 0, 1, -60, 8, {},
                            push=lambda *a: None, envelope=(None, 1, 1, 2, None))


class _Encoder:
    def encode(self, audio, sr, hop):
        return torch.zeros(audio.shape[0], 9, 4)


class _Extractor:
    def extract(self, window, **kw):
        return torch.zeros(window.shape[0], 9)


class _Ctx:
    def volume_extract(self, audio, hop):
        return torch.zeros(audio.shape[0], 9)


def test_header_and_exports_agree(lib_path):
    import hipddsp
    header = open(os.path.join(ROOT, "include", "ddsp_amd.h")).read()
    lib = ctypes.CDLL(lib_path)
    for name, n in (("ddsp_envelope_rms", 14), ("ddsp_envelope_apply", 23)):
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
        assert len(proto.split(",")) == len(hipddsp.SIGNATURES[name][1]) == n and hasattr(lib, name), name
    assert hipddsp.load_library().ddsp_abi_version() == hipddsp.ABI_VERSION == 8             # new symbols beside unchanged ones
    common = open(os.path.join(ROOT, "ddsp-svc-official_amd", "csrc", "common.h")).read()
    assert "#define DDSP_DEV_ERR_ENVELOPE 9 " in common and "#define DDSP_DEV_ERR_RETRIEVE 8 " in common
    for name in ("envelope_rms", "envelope_mix_"):
        assert callable(getattr(hipddsp.Context, name))
    for text in ("change_rms", "SILENT SOURCE SILENCES THE OUTPUT", "no smoothing, no cap on the gain"):
        assert text in header
