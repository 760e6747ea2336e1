"""Offline conversion of JOBS - (file, model, speaker or mix, key) - host side (no GPU): `infer_offline.job_table` and
`job_groups`, the layout of the jobs in the one output (`stitch_plan_many` over jobs), the refusals that come before any launch,
the new symbols' place in the header, the ctypes table and the library, and the host checks of `Context.pcm16`'s spans."""
import ctypes
import inspect

import pytest

from infer_offline import job_groups, job_table, piece_table, stitch_plan_many
from test_bank_models_host import bank_model

BLOCK, SR = 512, 44100
# file 0: two slices (a silence between them), file 1: one, file 2: none
SLICES = [[(0, 20 * BLOCK), (30 * BLOCK, 57 * BLOCK)], [(BLOCK, 31 * BLOCK)], []]
# file 0 to all three models, at keys 0 and +3, with an id and with a mix; file 1 twice; the file without slices once
JOBS = [(0, 0, 1, 0), (0, 1, {1: 0.25, 3: 0.75}, 3), (1, 1, 2, 3), (0, 2, 2, 0), (1, 0, 1, -2.5), (2, 2, 1, 0)]


@pytest.fixture(scope="module")
def models(lib_path):
    return [bank_model("CombSub", 1, 43), bank_model("Sins", 3, 44), bank_model("CombSubFast", 2, 45)]


def test_job_table_rows_name_the_files_own_offsets(models):
    pieces = piece_table(SLICES, float(BLOCK))
    assert [row[0] for row in pieces] == [0, 0, 1]
    table = job_table(pieces, 3, JOBS, models)
    rows = table["rows"]
    assert [row[5] for row in rows] == [0, 0, 1, 1, 2, 3, 3, 4]                      # job after job; job 5 has no rows
    for row, i in zip(rows, table["piece_of_row"]):
        assert row[:5] == pieces[i]                                                  # the source columns are the file's own
    by_job = [[row[:5] for row in rows if row[5] == j] for j in range(len(JOBS))]
    assert by_job[0] == by_job[1] == by_job[3] == list(pieces[:2]) and by_job[2] == by_job[4] == [pieces[2]] and by_job[5] == []
    assert table["model_of_job"] == [0, 1, 1, 2, 0, 2]
    assert table["speakers"] == [1, {1: 0.25, 3: 0.75}, 2, 2, 1, 1]
    assert table["key_factor"] == [2 ** (key / 12) for _, _, _, key in JOBS] and table["key_factor"][0] == 1.0
    assert table["starts_per_job"] == [[0, 30], [0, 30], [1], [0, 30], [1], []]


def test_jobs_lie_in_job_order_at_even_bases(models):
    """The lengths a render without the enhancer gives (n_frames * block), one made odd: every job's base is even, the spans
    ascend in job order, nothing fades across jobs, and two jobs over one file have the same plan behind their bases."""
    pieces = piece_table(SLICES, float(BLOCK))
    table = job_table(pieces, 3, JOBS, models)
    lengths = [[pieces[i][2] * BLOCK + (1 if j == 0 and n == 1 else 0) for n, i in enumerate(idx)]
               for j, idx in enumerate([[i for row, i in zip(table["rows"], table["piece_of_row"]) if row[5] == j]
                                        for j in range(len(JOBS))])]
    spans, p, fade, total = stitch_plan_many(table["starts_per_job"], lengths, BLOCK, SR, SR)
    assert len(spans) == len(JOBS)
    end, at = 0, 0
    for j, (base, n) in enumerate(spans):
        assert base % 2 == 0 and end <= base <= end + 1, j
        if lengths[j]:
            assert fade[at] == 0, j
        at, end = at + len(lengths[j]), base + n
    assert total == end and spans[0][1] % 2 == 1 and spans[1][0] == spans[0][1] + 1   # an odd job: a gap of one sample
    assert spans[5][1] == 0
    assert [x - spans[1][0] for x in p[2:4]] == [x - spans[3][0] for x in p[5:7]]     # jobs 1 and 3: the same file, the same plan


def test_groups_are_numbered_model_by_model(models):
    """`noise_seed`: group g draws with seed + g * 2**32, and g counts `job_groups`' list - model 0's groups, then model 1's,
    then model 2's - whatever order the jobs name the models in."""
    pieces = piece_table(SLICES, float(BLOCK))
    table = job_table(pieces, 3, JOBS, models)
    for budget in (0, 64, 10000):
        groups = job_groups(table, 3, budget)
        assert [m for m, _ in groups] == sorted(m for m, _ in groups)
        assert sorted(i for _, g in groups for i in g) == list(range(len(table["rows"])))
        for m, g in groups:
            assert {table["model_of_job"][table["rows"][i][5]] for i in g} == {m}
            assert len(g) == 1 or len(g) * max(table["rows"][i][2] for i in g) <= budget
    assert [len(g) for _, g in job_groups(table, 3, 0)] == [1] * 8
    assert [(m, len(g)) for m, g in job_groups(table, 3, 10000)] == [(0, 3), (1, 3), (2, 2)]
    assert len([1 for m, _ in job_groups(table, 3, 64) if m == 1]) >= 2                # a model's rows in two groups
    # a model without jobs has no group and takes no number
    only = job_table(pieces, 3, [(0, 2, 1, 0)], models)
    assert [m for m, _ in job_groups(only, 3, 10000)] == [2]


@pytest.mark.parametrize("jobs,what", [
    ([(0, 3, 1, 0)], "model index 3"),
    ([(0, -1, 1, 0)], "model index -1"),
    ([(0, 0, 1, 0), (0, 2, 3, 0)], r"job 1: speaker id 3 is outside \[1, 2\] of models\[2\]"),
    ([(0, 0, 0, 0)], "speaker id 0"),
    ([(0, 1, {1: 0.5, 4: 0.5}, 0)], r"speaker id 4 is outside \[1, 3\]"),
    ([(0, 1, {}, 0)], "1 to 16 ids"),
    ([(3, 0, 1, 0)], "file 3"),
    ([(0, 0, 1)], "must be"),
    ([(0, 0, 1, "high")], "key"),
])
def test_job_table_refuses(models, jobs, what):
    with pytest.raises(ValueError, match=what):
        job_table(piece_table(SLICES, float(BLOCK)), 3, jobs, models)


def test_models_must_agree(models):
    pieces = piece_table(SLICES, float(BLOCK))
    with pytest.raises(ValueError, match=r"models\[2\].block_size is 256"):
        job_table(pieces, 3, JOBS[:1], [models[0], models[1], bank_model("CombSub", 1, 46, block_size=256)])
    with pytest.raises(ValueError, match=r"models\[1\].n_unit is 64"):
        job_table(pieces, 3, JOBS[:1], [models[0], bank_model("Sins", 3, 47, n_unit=64), bank_model("CombSub", 1, 46, block_size=256)])
    with pytest.raises(ValueError, match="non-empty list"):
        job_table(pieces, 3, JOBS[:1], [])


def test_convert_many_device_refuses_before_any_launch(models):
    """Nothing here has a device: a refusal that came after a launch would fail on the CPU models instead."""
    import numpy as np

    import infer_offline
    from ddsp.vocoder import DotDict
    args = DotDict({"data": {"block_size": BLOCK, "sampling_rate": SR}})
    audios = [np.zeros(4 * BLOCK, dtype=np.float32)]
    call = lambda *a, **kw: infer_offline.convert_many_device(models[0], args, audios, SR, None, None, *a, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="leave spk_ids"):
        call(1, jobs=[(0, 0, 1, 0)], models=models)
    with pytest.raises(ValueError, match="leave spk_ids"):
        call(jobs=[(0, 0, 1, 0)], models=models, keys=2)
    with pytest.raises(ValueError, match="model index 3"):
        call(jobs=[(0, 3, 1, 0)], models=models)
    with pytest.raises(ValueError, match="file 1"):
        call(jobs=[(1, 0, 1, 0)], models=models)
    with pytest.raises(ValueError, match=r"models\[1\].block_size"):
        call(jobs=[(0, 0, 1, 0)], models=[models[0], bank_model("CombSub", 1, 46, block_size=256)])
    with pytest.raises(ValueError, match="models\\[0\\] itself"):
        call(jobs=[(0, 0, 1, 0)], models=models[1:])
    with pytest.raises(ValueError, match="goes with jobs"):
        call(1, models=models)
    with pytest.raises(ValueError, match="required without jobs"):
        call()
    out, spans, sr = call(jobs=[], models=models)                      # CPU models: an empty list launches nothing
    assert out.numel() == 0 and spans == [] and sr == SR
    params = inspect.signature(infer_offline.convert_many_device).parameters
    assert params["jobs"].default is None and params["models"].default is None and params["spk_ids"].default is None


def test_new_symbols_are_declared_bound_and_exported(lib_path):
    import hipddsp
    from test_abi_fold_host import _declared
    lib = ctypes.CDLL(lib_path)
    for name, n_args in (("ddsp_pieces_gather_jobs", 19), ("ddsp_pcm16", 9)):
        assert hasattr(lib, name) and len(hipddsp.SIGNATURES[name][1]) == n_args and name in _declared()
    gather = inspect.getsource(hipddsp.Context.pieces_gather)
    assert gather.count("self.call(") == 1 and "ddsp_pieces_gather_jobs" in gather
    assert hasattr(hipddsp.Context, "pcm16") and hipddsp.ABI_VERSION == 8
