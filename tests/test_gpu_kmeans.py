"""Unit index reduction on the device: `ddsp_units_kmeans_assign` and `ddsp_units_kmeans_update` against their statement in numpy
fp64 and Python integers (tests/kmeans_cases.py), `UnitIndex.reduce` end to end, and `build_index.py`.

Bounds.  Integer cases (entries and centres in {-2..2}): every product and sum of a score is exact in fp32, so the assignment and
`moved` equal the statement's element for element, ties included.  Real data (`KC.separated_case`): the gap between the best and
the second-best fp64 score of EVERY entry is asserted, before the device is touched, to exceed twice `score_bound` of
tests/retrieval_cases.py (the worst-case fp32 error of one score); the ids then equal the statement's.  The update is exact in
fixed point: centres and counts equal the statement's bit for bit, and so does a whole reduction."""
import os

import numpy as np
import pytest
import torch

import kmeans_cases as KC
import retrieval_cases as RC

pytestmark = pytest.mark.gpu


def _i32(dev, a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev)


def _f32(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _assign(ctx, dev, vec, cen, previous=None):
    """-> (assignment, moved) of one call; previous: the assignment before it (None: all -1)."""
    v, c = _f32(dev, vec), _f32(dev, cen)
    a = torch.full((vec.shape[0],), -1, dtype=torch.int32, device=dev) if previous is None else _i32(dev, previous)
    moved = torch.zeros(1, dtype=torch.int32, device=dev)
    assert ctx.units_kmeans_assign_(v, c, ctx.units_index_norms(c), a, moved) is a
    torch.cuda.synchronize()
    return a.cpu().numpy(), int(moved.item())


def _update(ctx, dev, vec, a, cen, S):
    v, c = _f32(dev, vec), _f32(dev, cen)
    count = torch.full((cen.shape[0],), 77, dtype=torch.int32, device=dev)                   # (77, 7: every element is written)
    ws = torch.full((cen.size,), 7, dtype=torch.int64, device=dev)
    assert ctx.units_kmeans_update_(v, _i32(dev, a), c, count, S, ws) is c
    torch.cuda.synchronize()
    return c.cpu().numpy(), count.cpu().numpy()


# ---- 1. assign ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,C", KC.ASSIGN_SHAPES)
def test_assignment_is_exact_on_integers(ctx, dev, lib_path, N, K, C):
    vec, cen = KC.integer_case(N, K, C, seed=N + K)
    want = KC.assign(vec, cen)
    t = np.sort(RC.scores(vec, cen), axis=1)
    ties = int((t[:, 0] == t[:, 1]).sum()) if K > 1 else 0
    got, moved = _assign(ctx, dev, vec, cen)
    print(f"N {N} K {K} C {C}: {int((got != want).sum())} ids differ, {ties} entries tie for the best score, moved {moved}")
    assert np.array_equal(got, want) and moved == N                    # from all -1: every entry moves
    again, moved = _assign(ctx, dev, vec, cen, previous=got)           # the same centres: nothing moves
    assert np.array_equal(again, want) and moved == 0
    some = want.copy()
    some[::3] = (some[::3] + 1) % K if K > 1 else -1                   # a previous assignment that differs in every third place
    again, moved = _assign(ctx, dev, vec, cen, previous=some)
    assert np.array_equal(again, want) and moved == int((some != want).sum())


def test_every_row_twice_goes_to_the_smaller_id(ctx, dev, lib_path):
    vec, cen = KC.twice_case()
    got, moved = _assign(ctx, dev, vec, cen)
    want = KC.assign(vec, cen)
    assert np.array_equal(got, want) and moved == 64
    assert (got < 32).all() and (got[:32] == got[32:]).all()           # both copies of an entry, at the smaller of two equal centres
    assert (RC.scores(vec, cen)[np.arange(64), got] == RC.scores(vec, cen)[np.arange(64), got + 32]).all()   # (the ties are real)


def test_assignment_on_separated_real_data(ctx, dev, lib_path):
    vec, centres = KC.separated_case()
    gap, bound = KC.gap_condition(vec, centres)                        # asserts it for every entry, on the statement's side
    print(f"smallest gap between the best and the second score {gap:.3f}, worst-case fp32 error of a score {bound:.4f}")
    want = KC.assign(vec, centres)
    got, moved = _assign(ctx, dev, vec, centres)
    assert np.array_equal(got, want) and moved == 1500 and len(set(want.tolist())) == 40
    # the search kernel's answer to the same question: k = 1, ratio 1, on a copy of the entries, the centres as the index
    from infer_offline import UnitIndex, UnitIndexBank
    bank = UnitIndexBank([UnitIndex(centres)], device=dev, rows=1, frames=1500, k=1)
    ids = torch.full((1, 1500, 1), 77, dtype=torch.int32, device=dev)
    ctx.units_retrieve_(_f32(dev, vec)[None].clone(), bank, _i32(dev, [0]), _f32(dev, [1.0]), k=1, nn_id=ids)
    torch.cuda.synchronize()
    assert np.array_equal(ids.cpu().numpy()[0, :, 0], got)
    ctx.poll_error()


# ---- 2. update ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,C", KC.UPDATE_SHAPES)
def test_update_equals_the_statement_bit_for_bit(ctx, dev, lib_path, N, K, C):
    rng = np.random.default_rng(N)
    vec = (KC.integer_case(N, K, C, seed=N)[0] + rng.standard_normal((N, C)) * 0.37).astype(np.float32)   # (off the integers: real means)
    cen = KC.integer_case(N, K, C, seed=N + K)[1]
    a = KC.assign(vec, cen)
    S = KC.fixed_shift(vec)
    want, want_count = KC.update(vec, a, cen, S)
    got, count = _update(ctx, dev, vec, a, cen, S)
    assert KC.same_bits(got, want) and np.array_equal(count, want_count) and count.sum() == N
    again, count2 = _update(ctx, dev, vec, a, cen, S)                  # integer sums: the same bits on every run
    assert KC.same_bits(again, got) and np.array_equal(count2, count)


def test_update_none_empty_and_one_centre_for_all(ctx, dev, lib_path):
    N, K, C = 4099, 257, 256
    rng = np.random.default_rng(9)
    vec = (3 * rng.standard_normal((N, C))).astype(np.float32)
    cen = rng.standard_normal((K, C)).astype(np.float32)
    S = KC.fixed_shift(vec)
    a = (np.arange(N) // 7 % K).astype(np.int32)                       # runs of seven, as neighbouring frames come
    a[a == 100] = 3                                                    # centre 100 is empty
    a[5::11] = -1                                                      # "none", and ids outside [0, K): counted nowhere
    a[6::97] = K
    a[7::89] = 2 ** 31 - 1
    want, want_count = KC.update(vec, a, cen, S)
    got, count = _update(ctx, dev, vec, a, cen, S)
    assert KC.same_bits(got, want) and np.array_equal(count, want_count)
    assert count[100] == 0 and KC.same_bits(got[100], cen[100]) and count.sum() == int(((a >= 0) & (a < K)).sum()) < N
    # one centre holds all N entries: the worst contention and the largest sum (every entry at the largest magnitude)
    top = np.float32(np.abs(vec).max())
    vec = np.full((N, C), top, dtype=np.float32)
    vec[:, 1::2] = -top
    S = KC.fixed_shift(vec)
    assert N * abs(KC.fixed(top, S)) <= 2 ** 62 < 4 * N * abs(KC.fixed(top, S))              # within the bound, and near it
    a = np.full(N, 5, dtype=np.int32)
    want, want_count = KC.update(vec, a, cen, S)
    got, count = _update(ctx, dev, vec, a, cen, S)
    assert KC.same_bits(got, want) and np.array_equal(count, want_count) and count[5] == N
    assert KC.same_bits(got[5], vec[0]) and KC.same_bits(np.delete(got, 5, 0), np.delete(cen, 5, 0))


def test_the_binding_refuses_before_the_launch(ctx, dev, lib_path):
    vec, cen = KC.integer_case(7, 3, 36)
    v, c = _f32(dev, vec), _f32(dev, cen)
    n, a, m = ctx.units_index_norms(c), _i32(dev, [-1] * 7), _i32(dev, [0])
    for args in ((v.double(), c, n, a, m), (v, c[:, :32].contiguous(), n, a, m), (v, c, n[:2], a, m), (v, c, n, a.long(), m),
                 (v, c, n, a[:6], m), (v, c, n, a, _i32(dev, [0, 0])), (v, c, n, a.cpu(), m), (v[:2], c, n, a[:2], m),
                 (v, c, n.double(), a, m), (_f32(dev, np.zeros(7 * 36 + 1))[1:].view(7, 36), c, n, a, m),
                 (v, _f32(dev, np.zeros(3 * 36 + 1))[1:].view(3, 36), n, a, m)):       # contiguous, but 4 bytes off a 16-byte boundary
        with pytest.raises(ValueError, match="units_kmeans_assign_"):
            ctx.units_kmeans_assign_(*args)
    count, ws = _i32(dev, [0] * 3), torch.zeros(3 * 36, dtype=torch.int64, device=dev)
    for args in ((v, a, c, count, 40.0, ws), (v, a, c, count, True, ws), (v, a, c, count, 300, ws), (v, a, c, count, 40, ws[:-1]),
                 (v, a, c, count[:2], 40, ws), (v, a.long(), c, count, 40, ws), (v, a, c, count, 40, ws.cpu()),
                 (v, a, c, count, 40, ws.view(torch.int32)[1:]), (v, a, _f32(dev, np.zeros(3 * 36 + 1))[1:].view(3, 36), count, 40, ws)):
        with pytest.raises(ValueError, match="units_kmeans_update_"):
            ctx.units_kmeans_update_(*args)
    assert KC.same_bits(c.cpu().numpy(), cen) and a.tolist() == [-1] * 7 and m.item() == 0


# ---- 3. end to end --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def separated():
    """The separated data and its K = 40, 5-iteration reduction by the statement, the gap condition asserted at every iteration."""
    vec, _ = KC.separated_case()
    gaps = []
    kept, rep, cen = KC.reduce(vec, 40, 5, on_iteration=lambda c, a: gaps.append(KC.gap_condition(vec, c)))
    assert len(gaps) == 5
    return vec, kept, rep, cen, gaps


def test_reduce_equals_the_statement_bit_for_bit(ctx, dev, lib_path, separated):
    from infer_offline import UnitIndex
    vec, kept, want, cen, gaps = separated
    print("smallest gap / bound per iteration: " + ", ".join(f"{g:.3f} / {b:.4f}" for g, b in gaps))
    got, rep = UnitIndex(vec).reduce(40, iters=5, device=dev, report=True)
    assert KC.same_bits(got.vectors.numpy(), kept) and KC.same_bits(kept, cen[want["count"] > 0])
    assert np.array_equal(rep["count"], want["count"]) and rep["count"].dtype == np.int32 and rep["count"].sum() == 1500
    assert rep["moved"] == want["moved"] and rep["moved"][0] == 1500 and rep["dropped"] == want["dropped"]
    assert rep["shift"] == want["shift"] == KC.fixed_shift(vec)
    plain = UnitIndex(vec).reduce(40, iters=5, device=dev)
    assert isinstance(plain, UnitIndex) and torch.equal(plain.vectors, got.vectors)
    ctx.poll_error()


def test_reduce_drops_the_empty_centres(ctx, dev, lib_path):
    """Every row twice, K = N - 4: the copies' centres stay empty through every iteration and are left out at the end."""
    from infer_offline import UnitIndex
    half = (10 * np.random.default_rng(4).standard_normal((150, 36))).astype(np.float32)
    vec = np.concatenate([half, half])
    kept, want, _ = KC.reduce(vec, 296, 2)
    got, rep = UnitIndex(vec).reduce(296, iters=2, device=dev, report=True)
    assert want["dropped"] > 100 and rep["dropped"] == want["dropped"] and rep["moved"] == want["moved"]
    assert KC.same_bits(got.vectors.numpy(), kept) and np.array_equal(rep["count"], want["count"]) and len(got) == 296 - rep["dropped"]


def test_a_reduced_index_is_served_like_any_other(ctx, dev, lib_path, separated):
    from infer_offline import UnitIndex, UnitIndexBank
    vec, kept, _, _, _ = separated
    reduced = UnitIndex(vec).reduce(40, iters=5, device=dev)
    rng = np.random.default_rng(6)
    q = (vec[rng.integers(0, 1500, 2 * 9)] + 0.3 * rng.standard_normal((18, 256))).astype(np.float32).reshape(2, 9, 256)
    flat = q.reshape(-1, 256)
    assert RC.kth_gap(flat, kept, 4) > 4 * RC.score_bound(flat, kept)                        # the retrieval tests' condition, k = 4
    ratio = np.array([0.75, 0.4], dtype=np.float32)
    want, want_id, want_dist, _ = RC.retrieve_rows(q, [kept], [0, 0], ratio, 4)
    bank = UnitIndexBank([reduced], device=dev, rows=2, frames=9, k=4)
    got = _f32(dev, q)
    ids = torch.full((2, 9, 4), 77, dtype=torch.int32, device=dev)
    dist = torch.full((2, 9, 4), 7.0, dtype=torch.float32, device=dev)
    ctx.units_retrieve_(got, bank, _i32(dev, [0, 0]), _f32(dev, ratio), k=4, nn_id=ids, nn_dist=dist)
    torch.cuda.synchronize()
    got, ids, dist = got.cpu().numpy(), ids.cpu().numpy(), dist.cpu().numpy()
    tol = RC.blend_bound(kept)
    for b in range(2):
        for f in range(9):
            assert set(ids[b, f].tolist()) == set(want_id[b, f].tolist()), (b, f)
    assert np.abs(np.take_along_axis(dist, np.argsort(ids, axis=2), 2) -
                  np.take_along_axis(want_dist, np.argsort(want_id, axis=2), 2)).max() <= tol
    assert np.abs(got - want).max() <= tol
    ctx.poll_error()


def test_build_index_writes_the_file_that_load_reads(ctx, dev, lib_path, separated, tmp_path, capsys):
    import build_index
    from infer_offline import UnitIndex
    vec, kept, want, _, _ = separated
    os.makedirs(tmp_path / "units" / "3")
    np.save(tmp_path / "units" / "3" / "a.0.npy", vec[:700])           # two files, sorted by name, frame after frame
    np.save(tmp_path / "units" / "3" / "b.0.npy", vec[700:])
    out = str(tmp_path / "voice3.pt")
    assert build_index.main(["-i", str(tmp_path), "--spk", "3", "--centres", "40", "--iters", "5", "-o", out, "-d", str(dev)]) == 0
    assert KC.same_bits(UnitIndex.load(out).vectors.numpy(), kept)
    line = capsys.readouterr().out
    assert f"1500 entries in, {len(kept)} centres out, {want['dropped']} dropped, moved in the last iteration {want['moved'][-1]}" in line
    direct = UnitIndex.from_units_dir(str(tmp_path), spk=3, centres=40, iters=5, device=dev)
    assert KC.same_bits(direct.vectors.numpy(), kept)
