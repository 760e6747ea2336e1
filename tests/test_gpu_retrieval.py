"""Unit retrieval on the device: `ddsp_units_retrieve` against its numpy statement (tests/retrieval_cases.py), offline jobs with
an index, and `StreamBank(indices=...)`.

Bounds.  Integer cases (entries in {-2..2}, queries in {-3..3}): every product and sum of a score is exact in fp32, so `nn_id`
equals the statement's ids element for element, ties included.  Real data (the generator of `RC.real_case`): the gap between the
8th and the 9th fp64 score (0.062) is asserted to exceed four times the worst-case fp32 error of a score (0.014, |.| the Euclidean
norm of a vector) before the device is touched; ids then match as sets, and `nn_dist` and `out` are held within `RC.blend_bound` =
4 (C + 2) 2^-24 max|idx| (1.2e-3 there; seen: 4.2e-5 and 4.8e-7), the worst-case rounding of the direct fp32 distance carried
through the inverse square and the normalisation.  Elements the rule leaves alone:
their bits.  A job against the per-slice eager render over the statement's units: rms < `GATE` = 1e-4, the gate of the jobs
path elsewhere."""
import numpy as np
import pytest
import torch

import retrieval_cases as RC
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


def _bank_of(dev, indices, rows, Fr, k):
    from infer_offline import UnitIndex, UnitIndexBank
    return UnitIndexBank([UnitIndex(v) for v in indices], device=dev, rows=rows, frames=Fr, k=k)


# ---- 1. the kernels -------------------------------------------------------------------------------------------------------------
def _run(ctx, dev, units, indices, index_of_row, ratio_of_row, k, counts=None, bank=None, nn=True):
    rows, Fr, _ = units.shape
    bank = _bank_of(dev, indices, rows, Fr, k) if bank is None else bank
    got = _f32(dev, units)
    ids = torch.full((rows, Fr, k), 77, dtype=torch.int32, device=dev) if nn else None      # (77, 7: every element is written)
    dist = torch.full((rows, Fr, k), 7.0, dtype=torch.float32, device=dev) if nn else None
    out = ctx.units_retrieve_(got, bank, _i32(dev, index_of_row), _f32(dev, ratio_of_row), k=k,
                              n_frames=None if counts is None else _i32(dev, counts), nn_id=ids, nn_dist=dist)
    assert out is got
    torch.cuda.synchronize()
    return got.cpu().numpy(), None if ids is None else ids.cpu().numpy(), None if dist is None else dist.cpu().numpy()


def test_index_norms(ctx, dev, lib_path):
    vec, _ = RC.integer_case(333, 36, 1, 1, seed=8)
    nrm = ctx.units_index_norms(_f32(dev, vec)).cpu().numpy()
    assert np.array_equal(nrm, (vec.astype(np.float64) ** 2).sum(1).astype(np.float32))     # integers: exact
    idx, _ = RC.real_case()
    nrm = ctx.units_index_norms(_f32(dev, idx)).cpu().numpy()
    assert np.abs(nrm - (idx.astype(np.float64) ** 2).sum(1)).max() <= 258 * 2.0 ** -24 * float((idx.astype(np.float64) ** 2).sum(1).max())


@pytest.mark.parametrize("N,C,k,rows,Fr", RC.EXACT_SHAPES)
def test_selection_is_exact_on_integers(ctx, dev, lib_path, N, C, k, rows, Fr):
    vec, q = RC.integer_case(N, C, rows, Fr, seed=N)
    ratio = np.full(rows, 0.5, dtype=np.float32)
    want, want_id, want_dist, err = RC.retrieve_rows(q, [vec], np.zeros(rows, dtype=np.int32), ratio, k)
    got, ids, dist = _run(ctx, dev, q, [vec], np.zeros(rows, dtype=np.int32), ratio, k)
    ties = sum(len(set(np.round(t, 9))) < len(t) for t in RC.scores(q.reshape(-1, C), vec))
    print(f"N {N} C {C} k {k}: {int((ids != want_id).sum())} ids differ, {ties} of {rows * Fr} queries have tied scores, "
          f"largest |out - statement| {np.abs(got - want).max():.3e}")
    assert not err and np.array_equal(ids, want_id)
    assert np.array_equal(dist, want_dist.astype(np.float32))                               # integers: the direct distance is exact
    assert (ids[:, :, min(k, N):] == -1).all() and (ids[:, :, :min(k, N)] >= 0).all()
    assert np.isfinite(got).all() and np.abs(got - want).max() <= RC.blend_bound(vec)
    ctx.poll_error()


def test_copies_and_an_exact_hit(ctx, dev, lib_path):
    vec, q = RC.copies_case()
    got, ids, dist = _run(ctx, dev, q, [vec], [0], [1.0], 4)
    want, want_id, _, _ = RC.retrieve_rows(q, [vec], [0], [1.0], 4)
    assert np.array_equal(ids, want_id)
    for f in range(5):                      # the three copies of the nearest, ascending, then the lowest-id copy of the next
        assert ids[0, f, :3].tolist() == [f, f + 5, f + 10] and ids[0, f, 3] < 5 and ids[0, f, 3] != f
    assert np.abs(got - want).max() <= RC.blend_bound(vec)
    # a query that IS an entry: s = 0, the floor makes its weight large and finite
    vec, q = RC.integer_case(333, 36, 1, 3, seed=4)
    q[0, 1] = vec[17]
    got, ids, dist = _run(ctx, dev, q, [vec], [0], [1.0], 8)
    want, want_id, want_dist, _ = RC.retrieve_rows(q, [vec], [0], [1.0], 8)
    assert np.array_equal(ids, want_id) and ids[0, 1, 0] == 17 and dist[0, 1, 0] == 0 == want_dist[0, 1, 0]
    assert np.isfinite(got).all() and np.abs(got - want).max() <= RC.blend_bound(vec)
    assert np.abs(got[0, 1] - vec[17]).max() <= RC.blend_bound(vec)                         # ratio 1 on a hit: the entry itself


def test_selection_and_blend_on_real_data(ctx, dev, lib_path):
    idx, q = RC.real_case()
    flat = q.reshape(-1, 256)
    gap, bound = RC.kth_gap(flat, idx, 8), RC.score_bound(flat, idx)
    print(f"smallest gap between the 8th and 9th score {gap:.4f}, worst-case fp32 error of a score {bound:.4f}")
    assert gap > 4 * bound                                                                  # on the statement's side, before the device
    ratio = np.array([0.75, 0.4], dtype=np.float32)
    want, want_id, want_dist, _ = RC.retrieve_rows(q, [idx], [0, 0], ratio, 8)
    got, ids, dist = _run(ctx, dev, q, [idx], [0, 0], ratio, 8)
    tol = RC.blend_bound(idx)
    e_out, e_dist = float(np.abs(got - want).max()), float(np.abs(dist - want_dist).max())
    print(f"largest |nn_dist - statement| {e_dist:.3e}, largest |out - statement| {e_out:.3e}, bound {tol:.3e}")
    for b in range(2):
        for f in range(37):                                                                 # no query is left out
            assert set(ids[b, f].tolist()) == set(want_id[b, f].tolist()), (b, f)
    order = np.argsort(ids, axis=2)
    assert np.abs(np.take_along_axis(dist, order, 2) - np.take_along_axis(want_dist, np.argsort(want_id, axis=2), 2)).max() <= tol
    assert e_out <= tol
    ctx.poll_error()


def test_untouched_elements_keep_their_bits(ctx, dev, lib_path):
    vec, q = RC.integer_case(333, 36, 6, 37, seed=12)
    q[1, 3] = np.float32(np.nan)                                                            # bits that arithmetic would not keep
    q[4, 30] = np.float32(-0.0)
    index_of_row = np.array([0, -1, 0, 5, 0, 0], dtype=np.int32)                            # none, ratio 0, an id outside [0, X)
    ratio = np.array([0.5, 0.5, 0.0, 0.5, 1.0, 0.25], dtype=np.float32)
    counts = np.array([37, 37, 37, 37, 20, 1], dtype=np.int32)
    want, want_id, _, err = RC.retrieve_rows(q, [vec], index_of_row, ratio, 3, counts)
    got, ids, dist = _run(ctx, dev, q, [vec], index_of_row, ratio, 3, counts)
    assert not err and np.array_equal(ids, want_id)
    assert RC.same_bits(got[[1, 2, 3]], q[[1, 2, 3]]) and RC.same_bits(got[4, 20:], q[4, 20:]) and RC.same_bits(got[5, 1:], q[5, 1:])
    assert (ids[[1, 2, 3]] == -1).all() and (ids[4, 20:] == -1).all() and not dist[[1, 2, 3]].any()
    assert not RC.same_bits(got[0], q[0]) and np.abs(got[[0, 4, 5]][:, :1] - want[[0, 4, 5]][:, :1]).max() <= RC.blend_bound(vec)
    assert np.abs(got[0] - want[0]).max() <= RC.blend_bound(vec) and np.abs(got[4, :20] - want[4, :20]).max() <= RC.blend_bound(vec)
    ctx.poll_error()                                                                        # none of this is an error
    for bad in (np.nan, 1.5, -0.25, np.inf):
        r = ratio.copy()
        r[4] = bad
        want, want_id, _, err = RC.retrieve_rows(q, [vec], index_of_row, r, 3, counts)
        got, ids, _ = _run(ctx, dev, q, [vec], index_of_row, r, 3, counts)
        assert err and RC.same_bits(got[4], q[4]) and (ids[4] == -1).all()
        assert np.array_equal(ids, want_id) and np.abs(got[0] - want[0]).max() <= RC.blend_bound(vec)   # the others are served
        with pytest.raises(ValueError, match="ddsp_units_retrieve"):
            ctx.poll_error()
        ctx.poll_error()                                                                    # read and cleared: reported once
        r[1], index_of_row2 = bad, index_of_row.copy()                                      # a bad ratio on a row without an index:
        r[4] = 1.0                                                                          # nobody judges it
        _run(ctx, dev, q, [vec], index_of_row2, r, 3, counts)
        ctx.poll_error()


def test_a_bank_of_two_indices_serves_each_row_as_its_own_index_would(ctx, dev, lib_path):
    a, q = RC.integer_case(333, 36, 4, 37, seed=21)
    b = RC.integer_case(1200, 36, 1, 1, seed=22)[0]
    q = q + np.float32(0.25)                                                                # (off the integers: real weights)
    both = _bank_of(dev, [a, b], 4, 37, 8)
    which, ratio = np.array([0, 1, 0, 1], dtype=np.int32), np.array([0.5, 0.6, 0.7, 0.8], dtype=np.float32)
    got, ids, dist = _run(ctx, dev, q, None, which, ratio, 8, bank=both)
    for row in range(4):
        solo, solo_id, solo_dist = _run(ctx, dev, q[row:row + 1], [(a, b)[which[row]]], [0], ratio[row:row + 1], 8)
        assert RC.same_bits(got[row], solo[0]) and np.array_equal(ids[row], solo_id[0]) and RC.same_bits(dist[row], solo_dist[0]), row
    want, want_id, _, _ = RC.retrieve_rows(q, [a, b], which, ratio, 8)
    assert np.array_equal(ids, want_id) and np.abs(got - want).max() <= RC.blend_bound(b)


def test_one_run_under_capture_equals_the_eager_run(ctx, dev, lib_path):
    vec, q = RC.integer_case(4099, 256, 2, 70, seed=31)
    bank = _bank_of(dev, [vec], 2, 70, 8)
    which, ratio, counts = _i32(dev, [0, 0]), _f32(dev, [0.5, 1.0]), _i32(dev, [70, 41])
    eager, eager_id, _ = _run(ctx, dev, q, None, [0, 0], [0.5, 1.0], 8, [70, 41], bank=bank)
    static, ids = _f32(dev, q), torch.zeros(2, 70, 8, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ctx.units_retrieve_(static, bank, which, ratio, k=8, n_frames=counts, nn_id=ids)
    torch.cuda.synchronize()
    static.copy_(_f32(dev, q))                                         # (the capture itself launched nothing)
    graph.replay()
    torch.cuda.synchronize()
    assert RC.same_bits(static.cpu().numpy(), eager) and np.array_equal(ids.cpu().numpy(), eager_id)
    ctx.poll_error()


def test_the_binding_refuses_before_the_launch(ctx, dev, lib_path):
    vec, q = RC.integer_case(7, 36, 2, 5)
    bank = _bank_of(dev, [vec], 2, 5, 8)
    u, which, ratio = _f32(dev, q), _i32(dev, [0, 0]), _f32(dev, [0.5, 0.5])
    for args, kw in (((u.double(), bank, which, ratio), {}), ((u, bank, which.long(), ratio), {}), ((u, bank, which, ratio.double()), {}),
                     ((u, bank, which[:1], ratio), {}), ((u, bank, which, ratio), {"k": 0}), ((u, bank, which, ratio), {"k": 17}),
                     ((u, object(), which, ratio), {}), ((u[:, :, :32].contiguous(), bank, which, ratio), {}),
                     ((u, bank, which, ratio), {"nn_id": torch.zeros(2, 5, 4, dtype=torch.int32, device=dev)}),
                     ((u, bank, which.cpu(), ratio), {}), ((u, bank, which, ratio), {"n_frames": torch.ones(2, device=dev)})):
        with pytest.raises(ValueError):
            ctx.units_retrieve_(*args, **kw)
    with pytest.raises(ValueError, match="workspace"):
        ctx.units_retrieve_(_f32(dev, np.zeros((40, 400, 36))), bank, _i32(dev, [0] * 40), _f32(dev, [0.5] * 40))
    assert RC.same_bits(u.cpu().numpy(), q)


def test_a_row_table_names_the_setting_of_every_row(ctx, dev, lib_path):
    """`owner=`: the settings are a bank's slots, the rows a compact width's; a padding row (-1, or past J) keeps its bits."""
    vec, q = RC.integer_case(333, 36, 4, 9, seed=41)
    q = q + np.float32(0.25)
    bank = _bank_of(dev, [vec], 4, 9, 3)
    slots_index, slots_ratio = _i32(dev, [-1, 0, 0]), _f32(dev, [0.5, np.nan, 0.5])         # slot 1 is bad, and nobody names it
    owner = np.array([2, -1, 0, 7], dtype=np.int32)
    got = _f32(dev, q)
    ctx.units_retrieve_(got, bank, slots_index, slots_ratio, k=3, owner=_i32(dev, owner))
    torch.cuda.synchronize()
    ctx.poll_error()
    want = RC.retrieve_rows(q, [vec], [0, -1, -1, -1], [0.5, 0, 0, 0], 3)[0]
    got = got.cpu().numpy()
    assert RC.same_bits(got[1:], q[1:]) and not RC.same_bits(got[0], q[0]) and np.abs(got - want).max() <= RC.blend_bound(vec)


# ---- 2. jobs --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(dev, lib_path):
    return [bank_model("CombSub", 2, 43, dev), bank_model("Sins", 2, 44, dev)]


def _noise(dev, slices, jobs, seed=917):
    import infer_offline
    pieces = infer_offline.piece_table(slices, float(HOP))
    rng = np.random.Generator(np.random.PCG64(seed))
    return [[torch.from_numpy(rng.random(row[2] * HOP, dtype=np.float32)).to(dev) for row in pieces if row[0] == job[0]] for job in jobs]


def _voice(C, n, seed):
    return np.random.default_rng(seed).standard_normal((n, C)).astype(np.float32)


def test_jobs_with_an_index_end_to_end(dev, lib_path, models, encoder, extractor, monkeypatch):  # noqa: F811
    """Two files (1.3 s in two slices, 0.7 s), three jobs, every row a group of its own, injected noise.  Job 1 (CombSub over
    file 0) names index 1 at 0.6; the other two name none."""
    import hipddsp
    import infer_offline
    from infer_offline import UnitIndex, UnitIndexBank
    audios, slices = _files()
    files = infer_offline.analyse_many(_args(), audios, SR, slices, encoder, extractor, 0, None)
    C = int(files["units"][0].shape[-1])
    voices = [_voice(C, 150, 5), _voice(C, 333, 6) * 0.5]
    bank = UnitIndexBank([UnitIndex(v) for v in voices], device=dev)
    jobs = [(1, 1, 2, 3.0), (0, 0, 1, 0.0, None, None, (1, 0.6)), (0, 0, 1, -2.0, None, None, None)]
    noise = _noise(dev, slices, jobs)
    calls = []
    launch = hipddsp.Context.units_retrieve_

    def counted(self, units, *a, **kw):
        calls.append(tuple(units.shape))
        return launch(self, units, *a, **kw)
    monkeypatch.setattr(hipddsp.Context, "units_retrieve_", counted)
    run = lambda jj, **kw: infer_offline.convert_many_device(None, _args(), audios, SR, encoder, extractor, slices=slices, jobs=jj,  # noqa: E731
                                                             models=models, batch_frames=1, noise=noise, **kw)
    ref, ref_spans, _ = run([job[:4] for job in jobs])
    same, _, _ = run([job[:4] for job in jobs], indices=bank)
    assert not calls and torch.equal(ref, same)                        # without an index among the jobs nothing is launched
    got, spans, sr_o = run(jobs, indices=bank, retrieve_k=4)
    torch.cuda.synchronize()
    ctx = hipddsp.context_for(dev)
    ctx.poll_error()
    assert spans == ref_spans and sr_o == SR and len(calls) == 5
    span = lambda x, j: x[spans[j][0]:spans[j][0] + spans[j][1]]  # noqa: E731
    for j in (0, 2):                                                   # the jobs without an index keep their bits
        assert torch.equal(span(got, j), span(ref, j)) and float(span(ref, j).abs().max()) > 1e-3
    k, m, spk = jobs[1][:3]
    rows = [row for row in files["pieces"] if row[0] == k]
    segments, f0, volume = infer_offline.file_features(files, k)
    spk_id = torch.tensor([[spk]], dtype=torch.int64, device=dev)
    outs = []
    for i, ((start, units), row) in enumerate(zip(segments, rows)):
        cnt = units.shape[1]
        blended = RC.retrieve_rows(units.cpu().numpy(), voices, [1], [0.6], 4)[0]
        assert np.abs(blended - units.cpu().numpy()).max() > 1e-2
        with torch.no_grad():
            sig = models[m](_f32(dev, blended), f0[:, start:start + cnt], volume[:, start:start + cnt], spk_id, noise=noise[1][i][None])[0]
        ctx.volume_gate_rows_(sig, files["volume"], _i32(dev, [start]), _i32(dev, [cnt]), -60, HOP,
                              file_dev=_i32(dev, [k]), file_frames_dev=files["n_frames_dev"])
        outs.append(sig[:, :cnt * HOP])
    plan = infer_offline.stitch_plan_many([[r[1] for r in rows]], [[o.shape[-1] for o in outs]], HOP, SR, SR)
    want = ctx.stitch(outs, plan[1], plan[2], plan[3])
    e = rms((span(got, 1) - want).cpu())
    print(f"job 1 against the per-slice eager render over the statement's units: rms {e:.3e}")
    assert want.numel() == spans[1][1] and e < GATE and float(want.abs().max()) > 1e-3
    assert rms((span(got, 1) - span(ref, 1)).cpu()) > 1e-4             # the retrieval is heard
    with pytest.raises(ValueError, match="no indices="):
        run(jobs)
    with pytest.raises(ValueError, match="index"):
        run([jobs[0], jobs[1][:6] + ((2, 0.5),)], indices=bank)


# ---- 3. the bank ----------------------------------------------------------------------------------------------------------------
S, K = 3, 3
BLOCK_TIME, XFADE_TIME, BUFFER_NUM, THR = 0.1, 0.04, 4, -45.0       # the geometry of tests/test_gpu_formant.py


def _bank(model, dev, encoder, **kw):  # noqa: F811
    import realtime
    return realtime.StreamBank(model, S, SR, BLOCK_TIME, XFADE_TIME, dev, buffer_num=BUFFER_NUM, threshold_db=THR, max_mix=K,
                               units_encoder=encoder, f0_extractor="ac", f0_min=65, f0_max=800, f0_dither=False, **kw)


def _unit_bank(dev, voices):
    from infer_offline import UnitIndex, UnitIndexBank
    return UnitIndexBank([UnitIndex(v) for v in voices], device=dev)


def _block(k, bank, dev):
    rng = np.random.Generator(np.random.PCG64(720 + k))
    t = (np.arange(bank.block) + k * bank.block) / SR
    blocks = np.stack([0.2 * np.sin(2 * np.pi * f * t) + 0.005 * rng.standard_normal(bank.block) for f in (150.0, 215.0, 335.0)])
    z = synthetic.make_inputs(8200 + k, S, bank.frames)
    return {"blocks": torch.from_numpy(blocks.astype(np.float32)).to(dev), "noise": z["noise"].to(dev)}


def _push(bank, x, active=None):
    row = (lambda name: x[name]) if active is None else (lambda name: x[name][list(active)].contiguous())
    return bank.push_audio(row("blocks"), noise=row("noise"), **({} if active is None else {"active": active}))


def test_bank_retrieval_rows(dev, lib_path, encoder):  # noqa: F811
    model = synthetic.build_model("CombSub", seed=43, device=dev)[0]
    C = int(model.unit2ctrl.n_unit)
    voices = [_voice(C, 150, 5), _voice(C, 333, 6) * 0.5]
    bank, eager = _bank(model, dev, encoder, indices=_unit_bank(dev, voices), retrieve_k=4), \
        _bank(model, dev, encoder, indices=_unit_bank(dev, voices), retrieve_k=4, use_graph=False)
    plain = _bank(model, dev, encoder)
    assert plain.graph_builds == bank.graph_builds == 1 and eager.graph_builds == 0
    settings = {1: [(1, 1, 0.5)], 2: [(1, 0, 0.8), (2, 1, 1.0)], 3: [(2, None, 0.5)]}       # block -> [(slot, index, ratio)]
    state, ever = {0: None, 1: None, 2: None}, set()
    for k in range(4):
        for slot, index, ratio in settings.get(k, []):
            for b in (bank, eager):
                b.set_index(slot, index, ratio)
            state[slot] = None if index is None else (index, ratio)
            ever.add(slot)
        x = _block(k, plain, dev)
        a, b, c = _push(plain, x), _push(bank, x), _push(eager, x)
        torch.cuda.synchronize()
        assert torch.equal(b, c) and torch.equal(bank.last_signal, eager.last_signal) and torch.equal(bank.last_units, eager.last_units), k
        off = [s for s in range(S) if state[s] is None]
        never = [s for s in off if s not in ever]                      # (the played block cross-fades with the block before)
        assert torch.equal(bank.last_units[off], plain.last_units[off]) and torch.equal(a[never], b[never]), k   # a slot that is off: the plain bank's bits
        assert torch.equal(bank.last_signal[off], plain.last_signal[off]), k
        for s in range(S):
            if state[s] is not None:
                want = RC.retrieve_rows(plain.last_units[s:s + 1].cpu().numpy(), voices, [state[s][0]], [state[s][1]], 4)[0]
                err = np.abs(bank.last_units[s:s + 1].cpu().numpy() - want).max()
                both = np.concatenate([voices[state[s][0]], plain.last_units[s].cpu().numpy()])    # (the bound over entries AND queries)
                assert err <= RC.blend_bound(both), (k, s, err)
                assert not torch.equal(bank.last_units[s], plain.last_units[s])
    assert bank.graph_builds == 1 and eager.graph_builds == 0                              # `set_index` captured nothing
    assert bank.index_of_slot.tolist() == [-1, 0, -1]
    bank.reset(1)
    assert bank.index_of_slot.tolist() == [-1, -1, -1] and bank.ratio_of_slot.tolist() == [0, 0, 0] and bank.graph_builds == 1
    with pytest.raises(ValueError, match="without indices="):
        plain.set_index(0, 0)
    for bad in ((2, 0.5), (0, 1.5), (0, float("nan")), (-1, 0.5)):
        with pytest.raises(ValueError, match="set_index"):
            bank.set_index(0, *bad)
    import hipddsp
    hipddsp.context_for(dev).poll_error()


def test_bank_retrieval_with_active_widths(dev, lib_path, encoder):  # noqa: F811
    """`active_widths=(2,)`: slot 2 alone leaves the width a padding row, and a paused slot's rows are untouched."""
    model = synthetic.build_model("CombSub", seed=43, device=dev)[0]
    kw = dict(active_widths=(2,))
    plain = _bank(model, dev, encoder, **kw)
    C = int(model.unit2ctrl.n_unit)
    voices = [_voice(C, 150, 5), _voice(C, 333, 6) * 0.5]
    bank, eager = _bank(model, dev, encoder, indices=_unit_bank(dev, voices), **kw), \
        _bank(model, dev, encoder, indices=_unit_bank(dev, voices), use_graph=False, **kw)
    builds = bank.graph_builds
    for b in (bank, eager):
        b.set_index(2, 1, 0.7)
        b.set_index(1, 0, 0.9)                                                             # slot 1 is never active: paused
    for k, active in enumerate(([0, 2], [2], [0, 2], [2])):                                # ([2] at width 2: a padding row)
        x = _block(k, plain, dev)
        window_1 = bank.windows[1].clone()
        a, b, c = _push(plain, x, active), _push(bank, x, active), _push(eager, x, active)
        torch.cuda.synchronize()
        assert torch.equal(b, c) and torch.equal(bank.last_units, eager.last_units) and b.shape[0] == len(active), k
        if len(active) == 2:
            assert torch.equal(a[0], b[0]) and torch.equal(plain.last_units[0], bank.last_units[0]), k
        assert not torch.equal(plain.last_units[-1], bank.last_units[-1]) and torch.isfinite(b).all(), k
        assert torch.equal(bank.windows[1], window_1) and bank.index_of_slot.tolist() == [-1, 0, 1], k
    assert bank.graph_builds == builds
    import hipddsp
    hipddsp.context_for(dev).poll_error()


def test_one_workspace_serves_every_width_of_a_bank(ctx, dev, lib_path, encoder):  # noqa: F811
    """The chunk count of a call falls as its rows grow, in steps (a ceil), so rows * chunks is NOT monotone: with 10 000 entries
    a call of 13 rows writes more candidates than one of 16.  The size `units_retrieve_workspace` gives grows with the rows
    all the same, and a bank reserved for 16 rows serves every narrower call - a stream bank's ladder of widths."""
    Fr, k, N = 87, 8, 10_000
    sizes = [ctx.units_retrieve_workspace(r, Fr, k, N) for r in range(1, 17)]
    assert sizes == sorted(sizes) and sizes[0] >= Fr * k * 8
    vec = _voice(36, N, 9)
    bank = _bank_of(dev, [vec], 16, Fr, k)
    q = _voice(36, 16 * Fr, 10).reshape(16, Fr, 36)
    whole = _run(ctx, dev, q, None, [0] * 16, [0.5] * 16, k, bank=bank)
    for r in (1, 2, 10, 12, 13, 14, 15):                               # every row is what it is in the full call, to the bit
        part = _run(ctx, dev, q[:r], None, [0] * r, [0.5] * r, k, bank=bank)
        assert RC.same_bits(part[0], whole[0][:r]) and np.array_equal(part[1], whole[1][:r]), r
    # the stream bank: three slots, a compact width of two, an index large enough for the widths to differ in chunks
    model = synthetic.build_model("CombSub", seed=43, device=dev)[0]
    voices = [_voice(int(model.unit2ctrl.n_unit), 12_000, 11)]
    kw = dict(active_widths=(2,))
    graph, eager = _bank(model, dev, encoder, indices=_unit_bank(dev, voices), **kw), \
        _bank(model, dev, encoder, indices=_unit_bank(dev, voices), use_graph=False, **kw)
    for b in (graph, eager):
        b.set_index(2, 0, 0.6)
    for n, active in enumerate(([0, 2], [2], None)):
        x = _block(n, graph, dev)
        got, want = _push(graph, x, active), _push(eager, x, active)
        torch.cuda.synchronize()
        assert torch.equal(got, want) and torch.equal(graph.last_units, eager.last_units) and torch.isfinite(got).all(), n
    with pytest.raises(ValueError, match="channels"):
        _bank(model, dev, encoder, indices=_unit_bank(dev, [_voice(36, 10, 1)]))
    import hipddsp
    hipddsp.context_for(dev).poll_error()


def test_bank_retrieval_with_models(dev, lib_path, encoder):  # noqa: F811
    """The retrieval sits in the shared analysis, in front of the per-model row gather: a bank with `models=` takes it, and a
    slot's units are what the single-model bank's are."""
    m0, m1 = bank_model("CombSub", 2, 43, dev), bank_model("Sins", 2, 44, dev)
    C = int(m0.unit2ctrl.n_unit)
    voices = [_voice(C, 150, 5), _voice(C, 333, 6) * 0.5]
    two = _bank(None, dev, encoder, models=[m0, m1], indices=_unit_bank(dev, voices))
    one = _bank(m0, dev, encoder, indices=_unit_bank(dev, voices))
    builds = two.graph_builds
    two.set_model(1, 1)
    for b in (one, two):
        b.set_index(1, 0, 0.5)
        b.set_index(2, 1, 1.0)
    for k in range(3):
        x = _block(k, one, dev)
        got, want = _push(two, x), _push(one, x)
        torch.cuda.synchronize()
        assert torch.equal(two.last_units, one.last_units) and torch.isfinite(got).all() and float(got.abs().max()) > 0, k
        assert torch.equal(got[[0, 2]], want[[0, 2]]), k                                   # (slots 0 and 2 render with model 0 in both)
    assert two.graph_builds == builds
