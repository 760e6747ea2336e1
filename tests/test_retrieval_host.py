"""Unit retrieval, host side (no GPU): the numpy statement (tests/retrieval_cases.py) against a naive loop, `UnitIndex` and its
files, jobs of four to seven entries, `job_indices` and `index_tables`, the symbols and the binding's table."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import retrieval_cases as RC
from conftest import ROOT
from test_bank_models_host import bank_model


# ---- the statement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,k", [(1, 4, 3), (5, 4, 3), (9, 8, 9), (12, 8, 4)])
def test_the_statement_equals_a_naive_loop(N, C, k):
    rng = np.random.default_rng(N)
    vec, q = rng.standard_normal((N, C)).astype(np.float32), rng.standard_normal((2, 3, C)).astype(np.float32)
    out, ids, dist, err = RC.retrieve_rows(q, [vec], [0, 0], [0.3, 1.0], k)
    assert not err
    for b, r in enumerate((0.3, 1.0)):
        for f in range(3):
            want, chosen, s = RC.naive_frame(q[b, f], vec, k, np.float32(r))
            n = min(k, N)
            assert ids[b, f, :n].tolist() == chosen and (ids[b, f, n:] == -1).all() and not dist[b, f, n:].any()
            assert np.allclose(dist[b, f, :n], s, rtol=1e-12) and np.allclose(out[b, f], want.astype(np.float32), atol=1e-6)


def test_ties_go_to_the_smaller_id_and_a_hit_is_finite():
    vec, q = RC.copies_case()
    out, ids, dist, _ = RC.retrieve_rows(q, [vec], [0], [1.0], 4)
    for f in range(5):
        assert ids[0, f, :3].tolist() == [f, f + 5, f + 10] and ids[0, f, 3] < 5 and ids[0, f, 3] != f
    vec, q = RC.integer_case(40, 8, 1, 2, seed=1)
    q[0, 0] = vec[7]
    out, ids, dist, _ = RC.retrieve_rows(q, [vec], [0], [1.0], 4)
    first = min(i for i in range(40) if np.array_equal(vec[i], vec[7]))
    assert ids[0, 0, 0] == first and dist[0, 0, 0] == 0 and np.isfinite(out).all() and np.allclose(out[0, 0], vec[7], atol=1e-6)


def test_what_keeps_its_bits():
    vec, q = RC.integer_case(20, 8, 5, 6, seed=2)
    q[1, 2] = np.float32(np.nan)
    out, ids, _, err = RC.retrieve_rows(q, [vec], [-1, 3, 0, 0, 0], [0.5, 0.5, 0.0, 0.5, np.nan], 3, [6, 6, 6, 2, 6])
    assert err and RC.same_bits(out[[0, 1, 2, 4]], q[[0, 1, 2, 4]]) and RC.same_bits(out[3, 2:], q[3, 2:])
    assert not RC.same_bits(out[3, :2], q[3, :2]) and (ids[[0, 1, 2, 4]] == -1).all() and (ids[3, :2] >= 0).all()
    assert not RC.retrieve_rows(q, [vec], [-1, 3, 0, 0, -1], [np.nan, 7.0, 0.0, 0.5, np.nan], 3)[3]   # judged only with an index


def test_the_real_generator_holds_its_condition():
    idx, q = RC.real_case()
    gap, bound = RC.kth_gap(q.reshape(-1, 256), idx, 8), RC.score_bound(q.reshape(-1, 256), idx)
    assert abs(gap - 0.062) < 1e-3 and abs(bound - 0.014) < 1e-3 and gap > 4 * bound


# ---- UnitIndex ---------------------------------------------------------------------------------------------------------------------
def test_unit_index_validation_and_files(tmp_path):
    from infer_offline import UnitIndex
    v = np.arange(40, dtype=np.float64).reshape(5, 8)
    idx = UnitIndex(v)
    assert len(idx) == 5 and idx.channels == 8 and idx.vectors.dtype == torch.float32 and idx.vectors.is_contiguous()
    for bad in (np.zeros((0, 8)), np.zeros((3, 6)), np.zeros((3, 1028)), np.zeros(8), np.zeros((2, 8), dtype=np.int64),
                np.full((2, 8), np.nan)):
        with pytest.raises(ValueError, match="UnitIndex"):
            UnitIndex(bad)
    path = str(tmp_path / "voice.pt")
    idx.save(path)
    assert torch.equal(UnitIndex.load(path).vectors, idx.vectors)
    torch.save({"other": 1}, path)
    with pytest.raises(ValueError, match="vectors"):
        UnitIndex.load(path)
    # the tree preprocess.py writes: units/<spk>/<name>.0.npy
    for spk, name, n in (("1", "a", 3), ("1", "b", 4), ("2", "c", 5)):
        os.makedirs(tmp_path / "units" / spk, exist_ok=True)
        np.save(tmp_path / "units" / spk / f"{name}.0.npy", np.full((n, 8), float(ord(name)), dtype=np.float32) + np.arange(n)[:, None])
    one = UnitIndex.from_units_dir(str(tmp_path), spk=1)
    assert len(one) == 7 and one.vectors[:, 0].tolist() == [97, 98, 99, 98, 99, 100, 101]
    assert len(UnitIndex.from_units_dir(str(tmp_path))) == 12
    few = UnitIndex.from_units_dir(str(tmp_path), spk=1, max_entries=3)                      # rows floor(i * 7 / 3) = 0, 2, 4
    assert few.vectors[:, 0].tolist() == [97, 99, 99] and len(UnitIndex.from_units_dir(str(tmp_path), spk=1, max_entries=9)) == 7
    with pytest.raises(ValueError, match="no .npy"):
        UnitIndex.from_units_dir(str(tmp_path), spk=3)
    with pytest.raises(ValueError, match="max_entries"):
        UnitIndex.from_units_dir(str(tmp_path), max_entries=0)


def test_unit_index_bank_refuses_before_the_device():
    from infer_offline import UnitIndex, UnitIndexBank
    a, b = UnitIndex(np.zeros((3, 8))), UnitIndex(np.zeros((3, 12)))
    for args, kw in ((([],), {}), (([a, "x"],), {}), (([a, b],), {}), (([a],), {"k": 17}), (([a],), {"rows": 0}), ((a,), {})):
        with pytest.raises(ValueError, match="UnitIndexBank"):
            UnitIndexBank(*args, **kw)


# ---- jobs --------------------------------------------------------------------------------------------------------------------------
def test_job_table_takes_a_seventh_entry():
    import infer_offline
    from infer_offline import PitchTune, job_indices, index_tables, job_table
    models = [bank_model("CombSub", 2, 43, "cpu")]
    pieces = [(0, 0, 10, 0, 5120), (1, 0, 8, 0, 4096)]
    tune = PitchTune(["A"])
    jobs = [(0, 0, 1, 0.0), (1, 0, 2, 1.0, 2.0), (0, 0, 1, 0.0, None, tune), (1, 0, 1, 0.0, None, None, (1, 0.25)),
            (0, 0, 1, 0.0, 1.0, tune, None)]
    table = job_table(pieces, 2, jobs, models, 2)
    assert table == job_table(pieces, 2, [j[:6] for j in jobs], models)                    # the tables do not hold it
    assert [len(j) for j in jobs[:3]] == [4, 5, 6] and job_indices(jobs) == [None, None, None, (1, 0.25), None]
    assert infer_offline.job_tunes(jobs) == [None, None, tune, None, tune] and infer_offline.job_formants(jobs)[4] == 1.0
    index, ratio = index_tables(job_indices(jobs))
    assert index.dtype == torch.int32 and index.tolist() == [-1, -1, -1, 1, -1] and ratio.dtype == torch.float32
    assert ratio.tolist() == [0, 0, 0, 0.25, 0]
    job_table(pieces, 2, [(0, 0, 1, 0.0, None, None, (5, 1))], models)                      # (no bank known: any index number >= 0)
    for bad in ((2, 0.5), (-1, 0.5), (0, 1.5), (0, -0.1), (0, float("nan")), (0.0, 0.5), (True, 0.5), (0,), "0:0.5", (0, "1")):
        with pytest.raises(ValueError, match="job 1: index"):
            job_table(pieces, 2, [jobs[0], (0, 0, 1, 0.0, None, None, bad)], models, 2)
    with pytest.raises(ValueError, match="job 0 must be"):
        job_table(pieces, 2, [(0, 0, 1, 0.0, None, None, None, None)], models)


def test_main_takes_an_index(tmp_path):
    import main
    from infer_offline import PitchTune, UnitIndex, job_table
    base = ["-m", "m.pt", "-i", "in.wav", "-o", "out.wav"]
    plain = main.parse_args(base)
    assert not hasattr(plain, "index") and not hasattr(plain, "index_ratio")
    cmd = main.parse_args(base + ["--index", "voice.pt", "--index_ratio", "0.75"])
    assert (cmd.index, cmd.index_ratio) == ("voice.pt", "0.75")
    assert main._job_entry(0, {"id": 2, "key": 3, "index": "a.pt", "index_ratio": 0.3, "suffix": "a"}) == (2, 3.0)
    with pytest.raises(ValueError, match="entry 1"):
        main._job_entry(1, {"id": 2, "index_rate": 0.3, "suffix": "a"})
    a, b = str(tmp_path / "a.pt"), str(tmp_path / "b.pt")
    UnitIndex(np.ones((3, 8))).save(a)
    UnitIndex(np.zeros((5, 8))).save(b)
    files = main._IndexFiles("cpu")
    assert files.setting("--index", None, 0.5) is None and files.bank() is None and not files.paths
    assert files.setting("--index", b, "0.75") == (0, 0.75) and files.setting("x", a, 0.5) == (1, 0.5)
    assert files.setting("x", b, 1) == (0, 1.0) and [len(i) for i in files.indices] == [5, 3]   # numbered as first named, loaded once
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="entry 4: index"):
            files.setting("--jobs: entry 4", a, bad)
    # the job as job_table takes it: a record per file, with None for every control the voice does not carry
    tune, Job = PitchTune(["A"]), main.Job
    e = main._cmd_envelope(main.parse_args(base + ["--rms_mix_rate", "0.25"]))

    def fields(voice):
        (job,) = main._file_jobs(1, [voice])
        return (job.file, job.model, job.spk, job.key, job.formant, job.tune, job.index, job.envelope)
    assert fields(Job(None, 1, 2, 3.0)) == (0, 1, 2, 3.0, None, None, None, None)
    assert fields(Job(None, 1, 2, 3.0, 1.0)) == (0, 1, 2, 3.0, 1.0, None, None, None)
    assert fields(Job(None, 1, 2, 3.0, None, tune)) == (0, 1, 2, 3.0, None, tune, None, None)
    assert fields(Job(None, 1, 2, 3.0, index=(1, 0.5))) == (0, 1, 2, 3.0, None, None, (1, 0.5), None)
    assert fields(Job(None, 1, 2, 3.0, envelope=e)) == (0, 1, 2, 3.0, None, None, None, e)
    assert [j.file for j in main._file_jobs(3, [Job(None, 0, 1, 0.0), Job(None, 0, 2, 0.0)])] == [0, 0, 1, 1, 2, 2]
    models = [bank_model("CombSub", 2, 43, "cpu")]
    jobs = main._file_jobs(1, [Job(None, 0, 1, 0.0, None, None, files.setting("x", a, 0.25)), Job(None, 0, 2, 1.0, 2.0, tune, None),
                               Job(None, 0, 1, 0.0), Job(None, 0, 1, 0.0, envelope=e)])
    job_table([(0, 0, 10, 0, 5120)], 1, jobs, models, len(files.indices))


# ---- the symbols -------------------------------------------------------------------------------------------------------------------
def test_header_and_exports_agree(lib_path):
    import hipddsp
    header = open(os.path.join(ROOT, "include", "ddsp_amd.h")).read()
    lib = ctypes.CDLL(lib_path)
    for name, n in (("ddsp_units_retrieve", 22), ("ddsp_units_retrieve_workspace", 6), ("ddsp_units_index_norms", 6)):
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
        assert len(proto.split(",")) == len(hipddsp.SIGNATURES[name][1]) == n and hasattr(lib, name), name
    declared = set(re.findall(r"\b(ddsp_\w+)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(hipddsp.SIGNATURES) and all(hasattr(lib, n) for n in declared)
    assert hipddsp.load_library().ddsp_abi_version() == hipddsp.ABI_VERSION == 8             # a new symbol beside unchanged ones
    common = open(os.path.join(ROOT, "ddsp-svc-official_amd", "csrc", "common.h")).read()
    assert f"#define DDSP_DEV_ERR_RETRIEVE {RC.ERR_RETRIEVE} " in common and "#define DDSP_DEV_ERR_TUNE 7 " in common
    assert hipddsp.MAX_RETRIEVE_K == 16


def test_the_entry_points_refuse_on_the_host():
    import graphed
    import inspect
    import infer_offline
    import realtime
    assert list(inspect.signature(graphed.block_chain).parameters)[-1] == "retrieve"
    assert list(inspect.signature(graphed.GraphedBlock.__init__).parameters)[-1] == "retrieve"
    p = inspect.signature(realtime.StreamBank.__init__).parameters
    assert p["indices"].default is None and p["retrieve_k"].default == 8
    p = inspect.signature(infer_offline.render_jobs_device).parameters
    assert p["indices"].default is None and "indices" not in inspect.signature(infer_offline.render_many_device).parameters
    with pytest.raises(ValueError, match="set_index"):
        infer_offline.check_job_index("StreamBank.set_index", (3, 0.5), 3)
    infer_offline.check_job_index("x", None)
