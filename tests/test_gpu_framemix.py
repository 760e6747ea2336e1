"""A speaker mix per FRAME on the device: `ddsp_unit2ctrl_fwd_framemix` (the embedding epilogue of the second prenet
convolution reads the weights of row m, not of m / Fr) against the reference's tensor-valued `spk_mix_dict`
(tests/golden/ref_framemix.npz), against the row mix, against the CPU oracle on both launches that carry the epilogue; a bad id;
`ddsp_mix_timeline` against its numpy statement (tests/test_framemix_host.py); timeline jobs through `convert_many_device`;
and a captured forward whose weights are rewritten between replays.

Bounds are quoted: the control matrix max < 2e-4 / rms < 2e-5 and the signal rms < 1e-4 (`GATE`) are what
tests/test_gpu_models.py holds its `mix` case to; a row of a ragged group against the row alone, and a job against its solo
call, rms < 1e-4 (`GATE` of tests/test_gpu_many.py, as tests/test_gpu_many_jobs.py uses it)."""
import os

import numpy as np
import pytest
import torch

import framemix_cases as FC
import synthetic
from conftest import GOLDEN, rms
from oracle import ctrlnet as OC
from test_bank_models_host import bank_model
from test_framemix_host import timeline_weights
from test_gpu_many import GATE, _voiced
from test_gpu_many import encoder  # noqa: F401  (the module-scoped random-weight HubertSoft fixture)
from test_gpu_many_jobs import _args, _files, extractor  # noqa: F401

pytestmark = pytest.mark.gpu
SR, HOP = synthetic.SR, synthetic.HOP


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "ref_framemix.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _tables(dev, w, ids=FC.IDS):
    """(ids (B, K) int32, w (B, Fr, K) fp32) on the device from a (B, Fr, K) array and one id per slot."""
    w = torch.as_tensor(w, dtype=torch.float32)
    return torch.tensor([list(ids)] * w.shape[0], dtype=torch.int32).to(dev), w.contiguous().to(dev)


# ---- 1. against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.NAMES)
def test_frame_mix_matches_the_reference(dev, lib_path, golden, name):
    """The reference's synthesisers with `spk_mix_dict = {id: (B, Frame, 1) tensor}` (ramps 1 -> 0 and 0 -> 1, a sine) on
    B = 3, Fr = 37: M = 111 rows, no multiple of a tile, batch rows inside tiles.  The per-frame tables and the tensor-valued
    dict are two spellings of one call.  (On the parent commit the pair is refused and the dict's tensors are read as floats.)"""
    model, cfg = synthetic.build_model(name, seed=int(golden["seed_weights"]), device=dev, n_spk=FC.N_SPK)
    inp = {k: v.to(dev) for k, v in synthetic.make_inputs(int(golden["seed_inputs"]), FC.B, FC.FR, n_spk=FC.N_SPK).items()}
    assert np.array_equal(golden["w"], FC.weights()) and tuple(golden["ids"]) == FC.IDS
    ids, w = _tables(dev, golden["w"])
    ctx = model._context(inp["f0"])
    with torch.no_grad():
        sig = model(inp["units"], inp["f0"], inp["volume"], inp["spk_id"], noise=inp["noise"], spk_mix_rows=(ids, w))[0]
        phase = model._scan(ctx, inp["f0"], None, True)["phase_frames"]
        ctrl = model.unit2ctrl.forward_flat(inp["units"], inp["f0"], phase, inp["volume"], inp["spk_id"], spk_mix_rows=(ids, w))
        as_dict = {i: w[:, :, k:k + 1].clone() for k, i in enumerate(FC.IDS)}
        sig_dict = model(inp["units"], inp["f0"], inp["volume"], inp["spk_id"], noise=inp["noise"], spk_mix_dict=as_dict)[0]
        if name != "Sins":          # (Sins keeps the reference's closed parameter list)
            sig_kw = model(inp["units"], inp["f0"], inp["volume"], inp["spk_id"], noise=inp["noise"], spk_mix_frames=(ids, w))[0]
            assert torch.equal(sig_kw, sig)
    assert torch.equal(sig_dict, sig)
    want_ctrl, want_sig = torch.from_numpy(golden[f"ctrl_{name}"]), torch.from_numpy(golden[f"signal_{name}"])
    d_ctrl = ctrl.cpu()[..., ::FC.CTRL_STEP] - want_ctrl
    e_sig = rms(sig.cpu()[:, ::FC.SIGNAL_STEP] - want_sig)
    print(f"{name}: ctrl max {float(d_ctrl.abs().max()):.3e} rms {rms(d_ctrl):.3e} (of {float(golden[f'ctrl_rms_{name}']):.3f}), "
          f"signal rms {e_sig:.3e} (of {float(golden[f'signal_rms_{name}']):.3f})")
    assert d_ctrl.abs().max() < 2e-4 and rms(d_ctrl) < 2e-5
    assert e_sig < 1e-4
    # the mix matters: the same call by plain id is far away
    with torch.no_grad():
        plain = model(inp["units"], inp["f0"], inp["volume"], inp["spk_id"], noise=inp["noise"])[0]
    assert rms((plain - sig).cpu()) > 1e-3


# ---- 2. against the row mix ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["CombSub", "CombSubFast"])
def test_constant_weights_are_the_row_mix(dev, lib_path, name):
    """Weights constant in time: the bits of `spk_mix_rows` with the same ids and weights, rectangular and ragged
    (n_frames = [37, 20, 1]); ragged rows are exactly 0 past their counts - whatever the weights hold there - and equal, at
    the ragged gate, to the row rendered alone at its own length."""
    model = bank_model(name, FC.N_SPK, 51, dev)
    B, Fr = FC.B, FC.FR
    inp = {k: v.to(dev) for k, v in synthetic.make_inputs(808, B, Fr, n_spk=FC.N_SPK).items()}
    row_w = torch.tensor([[0.25, 0.75, 0.0], [1.0, 0.0, 0.5], [0.3, 0.3, 0.3]])
    ids = torch.tensor([[2, 5, 8], [8, 1, 3], [4, 4, 1]], dtype=torch.int32).to(dev)
    rows = (ids, row_w.to(dev))
    frames = (ids, row_w[:, None, :].expand(B, Fr, 3).contiguous().to(dev))
    call = lambda **kw: model(inp["units"], inp["f0"], inp["volume"], inp["spk_id"], noise=inp["noise"], **kw)[0]  # noqa: E731
    with torch.no_grad():
        assert torch.equal(call(spk_mix_rows=frames), call(spk_mix_rows=rows))
        counts = [37, 20, 1]
        want = call(spk_mix_rows=rows, n_frames=counts)
        dirty = frames[1].clone()
        for b, n in enumerate(counts):
            dirty[b, n:] = float("nan")                         # the padding of the weights is never looked at
        got = call(spk_mix_rows=(ids, dirty), n_frames=counts)
        assert torch.equal(got, want) and torch.isfinite(got).all()
        for b, n in enumerate(counts):
            assert not got[b, n * HOP:].any() and float(got[b, :n * HOP].abs().max()) > 1e-4
            alone = model(inp["units"][b:b + 1, :n], inp["f0"][b:b + 1, :n], inp["volume"][b:b + 1, :n], inp["spk_id"][b:b + 1],
                          noise=inp["noise"][b:b + 1, :n * HOP], spk_mix_rows=(ids[b:b + 1], frames[1][b:b + 1, :n].contiguous()))[0]
            e = rms((got[b:b + 1, :n * HOP] - alone).cpu())
            print(f"{name} row {b} ({n} frames) against the row alone: rms {e:.3e}")
            assert e < GATE


# ---- 3. both launches that carry the epilogue ----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Fr", [(2, 53), (3, 172)])
def test_both_epilogue_launches_match_the_oracle(dev, lib_path, B, Fr):
    """`u2c_forward` (csrc/unit2ctrl_fwd.hip) runs the second prenet convolution as a K-split launch - four partial products into
    `kpart`, batch z == 0 adding bias and embeddings - when M = B * Fr <= KS_MAX_ROWS = 256 (n_unit = 256 satisfies the other
    conditions of `conv_split`), else as one whole-K launch.  (2, 53): M = 106, the K-split branch; (3, 172): M = 516, the plain
    one.  Against `oracle.ctrlnet.unit2control`, which broadcasts a (B, Fr, 1) weight as the reference does, at the
    control-network tolerance of tests/test_gpu_models.py (max < 2e-4, rms < 2e-5)."""
    model, cfg = synthetic.build_model("CombSub", seed=99)
    sd = {k[len("unit2ctrl."):]: v for k, v in model.state_dict().items() if k.startswith("unit2ctrl.")}
    inp = synthetic.make_inputs(4321 + B, B, Fr, with_noise=False)
    rng = np.random.Generator(np.random.PCG64(17 + B))
    phase = torch.from_numpy(rng.uniform(-np.pi, np.pi, (B, Fr)).astype(np.float32))
    w = torch.from_numpy(rng.uniform(-0.5, 1.0, (B, Fr, 3)).astype(np.float32))
    slots = (3, 100, 41)
    with torch.no_grad():
        want = OC.unit2control(sd, inp["units"], inp["f0"], phase, inp["volume"], inp["spk_id"],
                               {i: w[:, :, k:k + 1] for k, i in enumerate(slots)}, model.unit2ctrl.output_splits, return_flat=True)
        model = model.to(dev)
        ids, w_dev = _tables(dev, w, slots)
        got = model.unit2ctrl.forward_flat(inp["units"].to(dev), inp["f0"].to(dev), phase.to(dev), inp["volume"].to(dev), None,
                                           spk_mix_rows=(ids, w_dev)).cpu()
    err = got - want
    print(f"M = {B * Fr}: max {float(err.abs().max()):.3e} rms {rms(err):.3e}")
    assert got.shape == want.shape and err.abs().max() < 2e-4 and rms(err) < 2e-5


# ---- 4. a bad id -----------------------------------------------------------------------------------------------------------
def test_a_bad_id_raises_the_device_error(ctx, dev, lib_path):
    model = bank_model("CombSub", FC.N_SPK, 52, dev)
    inp = {k: v.to(dev) for k, v in synthetic.make_inputs(5, 2, 9, n_spk=FC.N_SPK).items()}
    ids, w = _tables(dev, np.full((2, 9, 2), 0.5, dtype=np.float32), (1, 2))
    torch.cuda.synchronize()
    ctx.poll_error()
    with torch.no_grad():
        good = model(inp["units"], inp["f0"], inp["volume"], None, noise=inp["noise"], spk_mix_rows=(ids, w))[0]
        for bad in (0, FC.N_SPK + 1, -3):
            broken = ids.clone()
            broken[1, 1] = bad
            out = model(inp["units"], inp["f0"], inp["volume"], None, noise=inp["noise"], spk_mix_rows=(broken, w))[0]
            torch.cuda.synchronize()
            assert torch.isfinite(out).all() and torch.equal(out[0], good[0])        # the slot adds nothing, the other row is untouched
            with pytest.raises(ValueError, match="spk_id"):
                ctx.poll_error()
            ctx.poll_error()                                                          # reported once


# ---- 5. the timeline kernel ------------------------------------------------------------------------------------------------
def test_mix_timeline_matches_the_numpy_statement(ctx, dev, lib_path):
    """3 jobs over 2 files, job 1 with a single breakpoint.  Job 0's breakpoints lie before the first piece (frame 2; the piece
    starts at 5), inside it (11), exactly on the second piece's first (30) and last (56) frame, and after the file's end (90);
    job 2 ramps over file 1 from inside its piece to behind its end.  N_max = 40 exceeds every row; one row names job -1, one
    job 3 = J.  Exact at breakpoints, on constant stretches and in the zero tail; at most 1 fp32 ulp elsewhere."""
    rows = [(0, 5, 15, 0, 0, 0), (0, 30, 27, 0, 0, 0), (1, 1, 30, 0, 0, 1), (1, 1, 30, 0, 0, 2), (0, 5, 15, 0, 0, -1),
            (0, 30, 27, 0, 0, 3), (0, 0, 1, 0, 0, 2)]
    J, K, N_max = 3, 3, 40
    bp_off = [0, 5, 6, 9]
    bp_frame = [2, 11, 30, 56, 90, 0, 4, 20, 64]
    rng = np.random.Generator(np.random.PCG64(33))
    bp_w = rng.uniform(-0.5, 1.5, (9, K)).astype(np.float32)
    bp_w[7] = bp_w[6]                                               # a constant stretch between two breakpoints (frames 4..20)
    job_ids = np.array([[2, 7, 1], [5, 1, 1], [8, 3, 4]], dtype=np.int32)
    i32 = lambda x: torch.tensor(np.asarray(x), dtype=torch.int32).to(dev)  # noqa: E731
    ids, w = ctx.mix_timeline(i32(rows), i32(bp_off), i32(bp_frame), torch.from_numpy(bp_w).to(dev), i32(job_ids), N_max)
    torch.cuda.synchronize()
    ctx.poll_error()                                                # a bad job is a padding row, not an error
    want_ids, want_w = timeline_weights(rows, J, bp_off, bp_frame, bp_w, job_ids, N_max)
    ids, w = ids.cpu().numpy(), w.cpu().numpy()
    assert ids.dtype == np.int32 and np.array_equal(ids, want_ids) and w.shape == (len(rows), N_max, K)
    assert ids[4].tolist() == [1, 1, 1] == ids[5].tolist() and not w[4].any() and not w[5].any()
    for r, (_, start, n, _, _, job) in enumerate(rows):
        assert not w[r, n:].any(), r                                # exact zeros, -0.0 excluded below
        assert not np.signbit(w[r, n:]).any(), r
    # exact at breakpoints ...
    assert np.array_equal(w[0, 6], bp_w[1]) and np.array_equal(w[1, 0], bp_w[2]) and np.array_equal(w[1, 26], bp_w[3])
    assert np.array_equal(w[3, 3], bp_w[6]) and np.array_equal(w[3, 19], bp_w[7])
    # ... and on constant stretches: one breakpoint, between two equal ones, before the first (job 2's row at file frame 0)
    assert all(np.array_equal(w[2, t], bp_w[5]) for t in range(30)) and all(np.array_equal(w[3, t], bp_w[6]) for t in range(3, 20))
    assert np.array_equal(w[6, 0], bp_w[6])
    # everywhere: at most one ulp from the fp64 statement rounded to fp32
    ulp = np.abs(w.view(np.int32).astype(np.int64) - want_w.view(np.int32).astype(np.int64))
    same_sign = np.signbit(w) == np.signbit(want_w)
    print("largest distance in ulp:", int(ulp[same_sign].max()), "exact:", float((ulp == 0).mean()))
    assert (same_sign | ((w == 0) & (want_w == 0))).all() and ulp[same_sign].max() <= 1
    exact = np.zeros(w.shape[:2], dtype=bool)
    exact[2], exact[4], exact[5], exact[3, 3:20] = True, True, True, True
    assert np.array_equal(w[exact], want_w[exact])
    # the ramps do change from frame to frame
    assert (np.abs(np.diff(w[0, :15, 0])) > 0).all() and (np.abs(np.diff(w[3, 20:30, 1])) > 0).all()


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------
def test_timeline_jobs_end_to_end(dev, lib_path, encoder, extractor):  # noqa: F811
    """Two synthetic files (1.3 s in two slices, 0.7 s) and two models.  Model 0: a timeline over file 0 - its second slice
    starts at file frame 77, so the breakpoints are met in file time -, an id job over file 1.  Model 1: an id and a mix job.
    Every row is a group of its own (batch_frames = 1) and the noise is injected.
      - the id job beside the timeline is rendered as a one-breakpoint timeline: against the call without any timeline
        (another speaker form of the control network), rms < GATE as tests/test_gpu_many_jobs.py holds an id beside a mix;
      - the timeline job against `render_device` of every piece with the tensor-valued `spk_mix_dict` built on the host from
        the numpy statement: rms < GATE;
      - model 1 has no timeline job: its spans are today's bits."""
    import infer_offline
    from infer_offline import SpeakerTimeline
    models = [bank_model("CombSub", 3, 43, dev), bank_model("CombSubFast", 2, 45, dev)]
    audios, slices = _files()
    tl = SpeakerTimeline([(0.2, 1), (0.45, {2: 0.6, 3: 0.4}), (1.0, {1: 0.5, 3: 0.5}), (1.25, 3)])
    jobs = [(0, 0, tl, 0), (1, 0, 2, 3), (0, 1, 1, 0), (1, 1, {1: 0.25, 2: 0.75}, -2)]
    plain = [(0, 0, 1, 0)] + jobs[1:]
    pieces = infer_offline.piece_table(slices, float(HOP))
    rng = np.random.Generator(np.random.PCG64(911))
    noise = [[torch.from_numpy(rng.random(row[2] * HOP, dtype=np.float32)).to(dev) for row in pieces if row[0] == k]
             for k, _, _, _ in jobs]
    run = lambda jj: infer_offline.convert_many_device(None, _args(), audios, SR, encoder, extractor, slices=slices, jobs=jj,  # noqa: E731
                                                       models=models, batch_frames=1, noise=noise)
    got, spans, sr_o = run(jobs)
    ref, ref_spans, _ = run(plain)
    torch.cuda.synchronize()
    infer_offline.hipddsp.context_for(dev).poll_error()
    assert spans == ref_spans and sr_o == SR
    span = lambda x, j: x[spans[j][0]:spans[j][0] + spans[j][1]]  # noqa: E731
    for j in (2, 3):
        assert torch.equal(span(got, j), span(ref, j)), j                           # no timeline on model 1: today's path
    e = rms((span(got, 1) - span(ref, 1)).cpu())
    print(f"the id job beside a timeline against the call without one: rms {e:.3e}")
    assert e < GATE and float(span(ref, 1).abs().max()) > 1e-3
    assert rms((span(got, 0) - span(ref, 0)).cpu()) > 1e-3                           # the glide is heard
    # the timeline job, piece by piece, from host-built weights
    files = infer_offline.analyse_many(_args(), audios, SR, slices, encoder, extractor, 0, None)
    segments, f0, volume = infer_offline.file_features(files, 0)
    off, frame, bp_w, job_ids = (t.numpy() for t in infer_offline.timeline_tables([tl], [0], SR, HOP))
    assert [s for s, _ in segments] == [0, 77] and frame.tolist() == [17, 39, 86, 108]
    mine = span(got, 0)
    for i, (start, units) in enumerate(segments):
        n = units.size(1)
        _, w = timeline_weights([(0, start, n, 0, 0, 0)], 1, off, frame, bp_w, job_ids, n)
        as_dict = {int(s): torch.from_numpy(w[:, :, k:k + 1].copy()).to(dev) for k, s in enumerate(job_ids[0])}
        want, _ = infer_offline.render_device(models[0], _args(), [(start, units)], f0, volume, None, spk_mix_dict=as_dict,
                                              noise=[noise[0][i]])
        a, b = start * HOP, (start + n) * HOP
        assert want.numel() == b and not want[:a].any()
        e = rms((mine[a:b] - want[a:b]).cpu())
        print(f"timeline piece {i} (file frames {start}..{start + n}): rms {e:.3e}")
        assert e < GATE and float(want[a:b].abs().max()) > 1e-3


# ---- 7. captured -----------------------------------------------------------------------------------------------------------
def test_a_captured_forward_follows_the_weights(dev, lib_path):
    """One capture, two replays with the weights rewritten between them, against two eager calls: the tables are read when the
    kernels run, nothing of the mix is a kernel argument."""
    import graphed
    model = bank_model("CombSubFast", FC.N_SPK, 53, dev)
    B, Fr = 2, 21
    inp = {k: v.to(dev) for k, v in synthetic.make_inputs(66, B, Fr, n_spk=FC.N_SPK).items()}
    rng = np.random.Generator(np.random.PCG64(67))
    first, second = (torch.from_numpy(rng.uniform(0, 1, (B, Fr, 2)).astype(np.float32)).to(dev) for _ in range(2))
    ids, w = _tables(dev, first.cpu(), (3, 8))
    call = lambda: model(inp["units"], inp["f0"], inp["volume"], None, noise=inp["noise"], spk_mix_rows=(ids, w))[0]  # noqa: E731

    class Captured(graphed._Captured):
        _run = staticmethod(call)

    with torch.no_grad():
        want = []
        for values in (first, second):
            w.copy_(values)
            want.append(call().clone())
        w.copy_(first)
        cap = Captured()
        out = cap._capture(dev, 2)
        got = []
        for values in (first, second):
            w.copy_(values)
            cap.graph.replay()
            got.append(out.clone())
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and not torch.equal(got[0], got[1])
