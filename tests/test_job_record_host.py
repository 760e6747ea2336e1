"""The `Job` record and the `controls` module, host side (no GPU): `Job.of` on tuples of four to eight entries and on records,
`job_table` and the four `job_*s` helpers on both forms, the tuple refusals with their texts, what a record is checked for, the
names `infer_offline` keeps, and that `controls` imports neither `infer_offline` nor `realtime`."""
import dataclasses
import subprocess
import sys

import pytest

import controls
import infer_offline
from conftest import PKG, ROOT
from controls import EnvelopeMix, FormantTimeline, Job, KeyTimeline, PitchTune, SpeakerTimeline
from infer_offline import job_envelopes, job_formants, job_indices, job_table, job_tunes
from test_bank_models_host import bank_model

FIELDS = ("file", "model", "spk", "key", "formant", "tune", "index", "envelope")
PIECES = [(0, 0, 10, 0, 5120), (1, 0, 8, 0, 4096)]


def _jobs():
    """The job list of test_envelope_host.test_job_table_takes_four_to_eight_entries - every length, a numeric formant, a tune,
    an index, an envelope - and behind it the three timelines, a mix dict and an integral formant (which `job_formants` floats)."""
    tune, a, b = PitchTune(["A"]), EnvelopeMix(0.25), EnvelopeMix(0.0)
    return [(0, 0, 1, 0.0), (1, 0, 2, 1.0, 2.0), (0, 0, 1, 0.0, None, tune), (1, 0, 1, 0.0, None, None, (1, 0.25)),
            (0, 0, 1, 0.0, None, None, None, a), (1, 0, 1, 0.0, 1.0, tune, (0, 0.5), b), (0, 0, 1, 0.0, None, None, None),
            (1, 0, SpeakerTimeline([(0.0, 1), (0.05, {1: 0.5, 2: 0.5})]), KeyTimeline([(0.0, 0.0), (0.05, 2.0)]),
             FormantTimeline([(0.0, -1.0), (0.05, 1.0)])), [0, 0, {1: 0.25, 2: 0.75}, -3, 2]]


def test_job_of_reads_every_length():
    for job in _jobs():
        got = Job.of(0, job)
        assert isinstance(got, Job) and [f.name for f in dataclasses.fields(Job)] == list(FIELDS)
        for n, name in enumerate(FIELDS):
            want = job[n] if n < len(job) else None
            assert getattr(got, name) is want or getattr(got, name) == want, (job, name)
        assert Job.of(3, got) is got                                                        # a record as it is
    assert sorted({len(job) for job in _jobs()}) == [4, 5, 6, 7, 8]
    assert Job(0, 1, 2, 3.0) == Job.of(0, (0, 1, 2, 3.0)) == Job(file=0, model=1, spk=2, key=3.0, formant=None, tune=None,
                                                                  index=None, envelope=None)


def test_job_table_and_the_lists_agree_on_both_forms():
    models = [bank_model("CombSub", 2, 43, "cpu")]
    jobs = _jobs()
    records = [Job.of(j, job) for j, job in enumerate(jobs)]
    table = job_table(PIECES, 2, jobs, models, 2)
    assert table == job_table(PIECES, 2, records, models, 2) == job_table(PIECES, 2, jobs[:3] + records[3:], models, 2)
    assert set(table) == {"rows", "piece_of_row", "model_of_job", "speakers", "key_factor", "starts_per_job", "keys"}
    assert table["model_of_job"] == [0] * 9 and table["speakers"][8] == {1: 0.25, 2: 0.75} and table["keys"][8] == -3.0
    assert table["key_factor"][1] == 2 ** (1.0 / 12) and table["key_factor"][7] is None
    for lists in (job_formants, job_tunes, job_indices, job_envelopes):
        assert lists(jobs) == lists(records), lists.__name__
    formants = job_formants(records)
    assert formants[:7] == [None, 2.0, None, None, None, 1.0, None] and formants[7] is jobs[7][4]
    assert formants[8] == 2.0 and type(formants[8]) is float                                 # (the int 2 of the last job)
    assert job_tunes(records)[5] is jobs[5][5] and job_indices(records)[3] == (1, 0.25) and job_envelopes(records)[4] is jobs[4][7]


def test_a_record_without_an_envelope_is_a_job_without_one():
    models = [bank_model("CombSub", 2, 43, "cpu")]
    job = Job(0, 0, 1, 0.0, envelope=None)
    assert job_table(PIECES, 2, [job], models) == job_table(PIECES, 2, [(0, 0, 1, 0.0)], models)
    assert job_envelopes([job]) == [None] and job_indices([job]) == [None] and job_formants([job]) == [None]


def test_the_tuple_refusals_keep_their_texts():
    models = [bank_model("CombSub", 2, 43, "cpu")]
    a = EnvelopeMix(0.25)
    must = (r"job_table: job 1 must be \(file, model_index, spk, key\), \(file, model_index, spk, key, formant\) or "
            r"\(file, model_index, spk, key, formant, tune\) with tune a PitchTune or None, or those six with "
            r"\(index_number, ratio\) or None behind them, or those seven with an EnvelopeMix behind them "
            r"\(a job without one is the shorter tuple\), got ")
    for bad in ((0, 0, 1), (0, 0, 1, 0.0, None, None, None, None), (0, 0, 1, 0.0, None, None, None, a, None),
                (0, 0, 1, 0.0, None, "A minor"), (0, 0, 1, 0.0, None, a), "0012", None, {0: 0}):
        for call in (lambda: Job.of(1, bad), lambda: job_table(PIECES, 2, [(0, 0, 1, 0.0), bad], models)):
            with pytest.raises(ValueError, match=must):
                call()
    for bad in (0.5, "0.5", (0.5,), {"rate": 0.5}):
        with pytest.raises(ValueError, match=r"job_table: job 1: envelope must be an EnvelopeMix, got "):
            Job.of(1, (0, 0, 1, 0.0, None, None, None, bad))
    with pytest.raises(ValueError, match=r"^render: job 2 must be "):
        Job.of(2, (0, 0), who="render")
    assert Job.of(0, (0, 0, 1, 0.0, None, None, None)).envelope is None                    # seven ending in None: accepted


def test_a_record_is_checked_before_any_launch():
    """`Job.of` hands a record on as it is, so `job_table` holds its tune and envelope to their types as it holds a tuple's."""
    models = [bank_model("CombSub", 2, 43, "cpu")]
    with pytest.raises(ValueError, match="job 0: tune must be a PitchTune or None"):
        job_table(PIECES, 2, [Job(0, 0, 1, 0.0, tune="A minor")], models)
    with pytest.raises(ValueError, match="job 1: envelope must be an EnvelopeMix"):
        job_table(PIECES, 2, [Job(0, 0, 1, 0.0), Job(0, 0, 1, 0.0, envelope=0.5)], models)
    with pytest.raises(ValueError, match="job 0: index"):
        job_table(PIECES, 2, [Job(0, 0, 1, 0.0, index=(2, 0.5))], models, 2)
    with pytest.raises(ValueError, match="job 0: file"):
        job_table(PIECES, 2, [Job(2, 0, 1, 0.0)], models)
    with pytest.raises(ValueError, match="share hop_seconds and frames"):
        job_table(PIECES, 2, [Job(0, 0, 1, 0.0, envelope=EnvelopeMix(0.5)), Job(0, 0, 1, 0.0, envelope=EnvelopeMix(0.5, 0.1))], models)


MOVED = ("SpeakerTimeline", "KeyTimeline", "FormantTimeline", "PitchTune", "UnitIndex", "UnitIndexBank", "EnvelopeMix",
         "timeline_tables", "key_tables", "formant_tables", "tune_tables", "index_tables", "envelope_tables", "check_job_index",
         "pitch_class", "SCALES", "NOTE_NAMES", "MAX_FORMANT", "Job", "job_formants", "job_tunes", "job_indices", "job_envelopes")


def test_infer_offline_keeps_every_name():
    import ddsp.analysis
    import realtime
    for name in MOVED:
        assert getattr(infer_offline, name) is getattr(controls, name), name
    for module in (realtime, infer_offline):
        assert module.MODEL_FIELDS is ddsp.analysis.MODEL_FIELDS and module._model_field is ddsp.analysis._model_field


def test_controls_imports_neither_converter():
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}]; import controls; "
            "print('LOADED', sorted(m for m in ('infer_offline', 'realtime', 'main') if m in sys.modules))")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "LOADED []" in out.stdout, out.stdout[-500:]
