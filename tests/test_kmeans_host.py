"""Unit index reduction, host side (no GPU): the statement (tests/kmeans_cases.py) against its loop-only form, the fixed point at
its edges, `iters = 0`, empty centres, the ValueErrors of `UnitIndex.reduce` / `from_units_dir`, `build_index.py`'s arguments and
the two symbols."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import kmeans_cases as KC
from conftest import ROOT


# ---- the statement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,C", [(1, 1, 4), (9, 3, 8), (20, 7, 4)])
def test_the_statement_equals_its_loops(N, K, C):
    rng = np.random.default_rng(N)
    vec = (rng.standard_normal((N, C)) * 3).astype(np.float32)
    cen = KC.init(vec, K)
    assert KC.same_bits(cen, vec[(np.arange(K) * N) // K])
    a = KC.assign(vec, cen)
    assert np.array_equal(a, KC.naive_assign(vec, cen)) and a.dtype == np.int32
    S = KC.fixed_shift(vec)
    a[0] = -1                                                          # "none" is counted nowhere
    got, count = KC.update(vec, a, cen, S)
    want, want_count = KC.naive_update(vec, a, cen, S)
    assert KC.same_bits(got, want) and np.array_equal(count, want_count) and count.sum() == N - 1
    for j in range(K):                                                 # the exact mean, rounded once to fp32 (S keeps every bit here)
        rows = np.nonzero(a == j)[0]
        if len(rows):
            assert np.allclose(got[j], vec[rows].astype(np.float64).mean(0), rtol=2.0 ** -23, atol=1e-12)


def _bound_holds(vec):
    S = KC.fixed_shift(vec)
    N = vec.shape[0]
    top = max(abs(KC.fixed(v, S)) for v in (vec.max(), vec.min()))
    assert N * top <= 2 ** 62, (S, N, top)
    return S


def test_fixed_shift_at_its_edges():
    zero = np.zeros((5, 4), dtype=np.float32)
    assert _bound_holds(zero) == 62 - 0 - 3
    assert KC.same_bits(KC.update(zero, np.zeros(5, dtype=np.int32), zero[:1].copy(), KC.fixed_shift(zero))[0], zero[:1])
    for top, E in ((1.0, 1), (0.5, 0), (4.0, 3), (np.float32(4.0) - np.float32(2.0 ** -21), 2), (2.0 ** -140, -139),
                   (float(np.finfo(np.float32).max), 128)):
        vec = np.full((3, 4), -top, dtype=np.float32)                  # a power of two is NOT below itself: E is one more
        assert math.frexp(float(top))[1] == E and _bound_holds(vec) == 62 - E - 2
    for N, L in ((1, 0), (2, 1), (1024, 10), (1025, 11), (4096, 12), (4097, 13)):
        vec = np.full((N, 4), 1.0, dtype=np.float32)
        assert (N - 1).bit_length() == L and _bound_holds(vec) == 62 - 1 - L
        if N > 1:                                                      # the bound is tight: one bit more would pass 2^63 at N = 2^L
            assert (1 << L) * abs(KC.fixed(1.0, 62 - 1 - L + 2)) >= 2 ** 63
    from infer_offline import UnitIndex
    for vec in (zero, np.full((1025, 4), 1.0, dtype=np.float32), np.full((3, 4), -0.5, dtype=np.float32)):
        assert UnitIndex.fixed_shift(torch.from_numpy(vec)) == KC.fixed_shift(vec)
    # the smallest S the rule can give, and the largest: what the entry point accepts
    assert 62 - 128 - 31 == -97 and 62 - (-148) - 0 == 210 and math.frexp(2.0 ** -149)[1] == -148


def test_iters_zero_is_the_max_entries_subset(tmp_path):
    from infer_offline import UnitIndex
    rng = np.random.default_rng(3)
    vec = rng.standard_normal((23, 8)).astype(np.float32)
    kept, rep, _ = KC.reduce(vec, 5, 0)
    assert KC.same_bits(kept, vec[(np.arange(5) * 23) // 5]) and rep["moved"] == [] and rep["dropped"] == 0
    os.makedirs(tmp_path / "units" / "1")
    np.save(tmp_path / "units" / "1" / "a.0.npy", vec)
    strided = UnitIndex.from_units_dir(str(tmp_path), spk=1, max_entries=5)
    got, rep = UnitIndex(vec).reduce(5, iters=0, device="cpu", report=True)                  # (no device is touched at iters = 0)
    assert torch.equal(got.vectors, strided.vectors) and KC.same_bits(got.vectors.numpy(), kept) and rep["moved"] == []
    assert torch.equal(UnitIndex.from_units_dir(str(tmp_path), centres=5, iters=0, device="cpu").vectors, strided.vectors)
    whole = UnitIndex(vec)
    assert whole.reduce(23, device="cpu") is whole and whole.reduce(400, iters=3, device="cpu") is whole
    assert whole.reduce(23, device="cpu", report=True)[1]["dropped"] == 0
    assert len(UnitIndex.from_units_dir(str(tmp_path), max_entries=7, centres=9, device="cpu")) == 7   # max_entries first


def test_an_empty_centre_is_kept_while_iterating_and_dropped_at_the_end():
    rng = np.random.default_rng(4)
    half = (10 * rng.standard_normal((6, 8))).astype(np.float32)
    vec = np.concatenate([half, half])                                 # rows i and i + 6 are copies
    seen = []
    kept, rep, cen = KC.reduce(vec, 12, 3, on_iteration=lambda c, a: seen.append((c.copy(), a.copy())))
    for c, a in seen:                                                  # every copy goes to the smaller id, in every iteration
        assert a.tolist() == list(range(6)) * 2 and c.shape == (12, 8)
    assert rep["count"].tolist() == [2] * 6 + [0] * 6 and rep["dropped"] == 6 and rep["moved"] == [12, 0, 0]
    assert KC.same_bits(cen[6:], vec[6:]) and KC.same_bits(kept, half)                       # kept their bits; the mean of two copies
    assert len(kept) == 6 and len(seen) == 3


def test_reduce_and_from_units_dir_refuse(tmp_path):
    from infer_offline import UnitIndex
    idx = UnitIndex(np.zeros((5, 8)))
    for bad in (0, -1, 2.0, True, None, "3"):
        with pytest.raises(ValueError, match="centres"):
            idx.reduce(bad)
    for bad in (-1, 1.5, False, None):
        with pytest.raises(ValueError, match="iters"):
            idx.reduce(3, iters=bad)
    os.makedirs(tmp_path / "units" / "1")
    np.save(tmp_path / "units" / "1" / "a.0.npy", np.zeros((5, 8), dtype=np.float32))
    for kw, what in (({"centres": 0}, "centres"), ({"centres": True}, "centres"), ({"centres": 2, "iters": -1}, "iters"),
                     ({"iters": None}, "iters"), ({"max_entries": 0}, "max_entries")):
        with pytest.raises(ValueError, match=what):
            UnitIndex.from_units_dir(str(tmp_path), **kw)
    with pytest.raises(RuntimeError, match="HIP device"):             # a reduction proper needs the device: no CPU fallback
        UnitIndex(np.arange(40, dtype=np.float32).reshape(10, 4)).reduce(3, iters=1, device="cpu")


def test_build_index_arguments(tmp_path, capsys):
    import build_index
    cmd = build_index.parse_args(["-i", "data", "-o", "v.pt"])
    assert (cmd.input, cmd.output, cmd.spk, cmd.centres, cmd.iters, cmd.max_entries) == ("data", "v.pt", None, 10000, 10, None)
    cmd = build_index.parse_args(["-i", "d", "-o", "v.pt", "--spk", "2", "--centres", "50", "--iters", "0", "--max_entries", "9"])
    assert (cmd.spk, cmd.centres, cmd.iters, cmd.max_entries) == ("2", 50, 0, 9)
    for bad in (["--centres", "0"], ["--iters", "-1"], ["--max_entries", "0"], ["--centres", "1.5"]):
        with pytest.raises(SystemExit):
            build_index.parse_args(["-i", "d", "-o", "v.pt"] + bad)
    with pytest.raises(SystemExit):
        build_index.parse_args(["-o", "v.pt"])
    capsys.readouterr()
    # a tree: up to the point where the device is needed, and through it when nothing is left to reduce
    from infer_offline import UnitIndex
    for spk, n in (("1", 4), ("2", 6)):
        os.makedirs(tmp_path / "units" / spk)
        np.save(tmp_path / "units" / spk / "a.0.npy", np.arange(n * 8, dtype=np.float32).reshape(n, 8) + 100 * int(spk))
    out = str(tmp_path / "voice.pt")
    assert build_index.main(["-i", str(tmp_path), "-o", out, "--spk", "2", "--centres", "3", "--iters", "0"]) == 0
    assert UnitIndex.load(out).vectors[:, 0].tolist() == [200.0, 216.0, 232.0]              # rows 0, 2, 4 of speaker 2
    assert "6 entries in, 3 centres out, 0 dropped, moved in the last iteration 0" in capsys.readouterr().out
    assert build_index.main(["-i", str(tmp_path), "-o", out, "-d", "cpu"]) == 0             # 10 rows, 10000 centres: saved as it is
    assert len(UnitIndex.load(out)) == 10
    with pytest.raises(RuntimeError, match="HIP device"):
        build_index.main(["-i", str(tmp_path), "-o", out, "--centres", "3", "-d", "cpu"])
    with pytest.raises(ValueError, match="no .npy"):
        build_index.main(["-i", str(tmp_path), "-o", out, "--spk", "9"])


# ---- the symbols -------------------------------------------------------------------------------------------------------------------
def test_both_symbols_are_declared_exported_and_bound(lib_path):
    import hipddsp
    header = open(os.path.join(ROOT, "include", "ddsp_amd.h")).read()
    lib = ctypes.CDLL(lib_path)
    for name, n in (("ddsp_units_kmeans_assign", 10), ("ddsp_units_kmeans_update", 12)):
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
        assert len(proto.split(",")) == len(hipddsp.SIGNATURES[name][1]) == n and hasattr(lib, name), name
    assert hipddsp.load_library().ddsp_abi_version() == hipddsp.ABI_VERSION == 8             # new symbols beside unchanged ones
    for method, name in (("units_kmeans_assign_", "ddsp_units_kmeans_assign"), ("units_kmeans_update_", "ddsp_units_kmeans_update")):
        import inspect
        src = inspect.getsource(getattr(hipddsp.Context, method))
        assert re.findall(r"call\(\s*\"(ddsp_\w+)\"", src) == [name]
    rule = header[header.index("UNIT INDEX REDUCTION"):header.index("int ddsp_units_kmeans_update(")]
    for words in ("floor(j * N / K)", "smaller centre id", "62 - E - L", "keeps its bits", "A definition of this project"):
        assert words in rule, words
