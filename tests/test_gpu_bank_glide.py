"""The speaker glide of `realtime.StreamBank(glide_breakpoints=...)` on the device: `ddsp_bank_glide` against its numpy statement
(`glide_ref` of tests/test_bank_glide_host.py); a bank that could glide and does not against the bank without the feature, bit for
bit; a timeline on one slot against the statement and against the eager per-frame forward; a paused slot; `set_speaker` and
`reset` on a gliding slot; the raw-audio form, where the launch is inside the captured block.

Geometry: S = 3 slots, `max_mix` = 3, 0.1 s blocks at the model's own 44.1 kHz (block 4410, window 22050 samples, 44 frames), the
`push_block` form with injected noise, no enhancer.  Weights: `synthetic.build_model('CombSub')` (n_spk = 100).

Exactness: weights equal the statement bit for bit at breakpoints, on held stretches, on slots without a timeline and on padding
rows; elsewhere within one fp32 ulp (the compiler may contract the fp64 multiply-add), as
`test_mix_timeline_matches_the_numpy_statement` allows."""
import numpy as np
import pytest
import torch

import synthetic
from infer_offline import SpeakerTimeline
from test_bank_glide_host import glide_ref, glide_state, set_points
from test_gpu_stream_bank import crepe, encoder  # noqa: F401  (the module-scoped tiny CREPE and random-weight HubertSoft fixtures)

pytestmark = pytest.mark.gpu
S, K, P_MAX, SR = 3, 3, 4, synthetic.SR
BLOCK_TIME, XFADE_TIME, BUFFER_NUM, THR = 0.1, 0.04, 4, -45.0
MIXES = [{2: 1.0}, {1: 0.3, 5: 0.7}, {7: 0.5, 3: 0.25, 4: 0.25}]
RAMP = [(0.15, 2), (0.25, {2: 0.5, 5: 0.5}), (0.35, {5: 0.7, 7: 0.3})]    # starts inside block 2, ends before block 5


@pytest.fixture(scope="module")
def model(dev, lib_path):
    return synthetic.build_model("CombSub", seed=43, device=dev)[0]


def _bank(model, dev, **kw):
    import realtime
    return realtime.StreamBank(model, S, SR, BLOCK_TIME, XFADE_TIME, dev, buffer_num=BUFFER_NUM, threshold_db=THR, max_mix=K, **kw)


def _inputs(k, bank, dev):
    """Block k of the three callers: blocks (S, block) of tones, units (S, Fr, 256), f0 (S, Fr, 1), noise (S, Fr * 512)."""
    rng = np.random.Generator(np.random.PCG64(700 + k))
    t = (np.arange(bank.block) + k * bank.block) / SR
    blocks = np.stack([0.2 * np.sin(2 * np.pi * f * t) + 0.01 * rng.standard_normal(bank.block) for f in (147.0, 220.0, 330.0)])
    z = synthetic.make_inputs(8100 + k, S, bank.frames)
    return {"blocks": torch.from_numpy(blocks.astype(np.float32)).to(dev), "units": z["units"].to(dev), "f0": z["f0"].to(dev),
            "noise": z["noise"].to(dev)}


def _push(bank, x, active=None):
    row = (lambda name: x[name]) if active is None else (lambda name: x[name][list(active)].contiguous())
    return bank.push_block(row("blocks"), row("units"), row("f0"), noise=row("noise"), **({} if active is None else {"active": active}))


def _state(bank):
    """The glide state of a bank as `glide_ref`'s keyword arguments (numpy copies)."""
    return {"clock": bank.glide_clock.cpu().numpy(), "bp_n": bank.glide_n.cpu().numpy(), "bp_t": bank.glide_t.cpu().numpy(),
            "bp_w": bank.glide_w.cpu().numpy(), "spk_w": bank.spk_w.cpu().numpy()}


def _exact_mask(rows, W, z, Fr, n_in, block, hop):
    """(W, Fr) bool: the frames at which the kernel owes the statement's bits - padding rows, slots without a timeline, frames
    before the first or from the last breakpoint on, and frames whose time is a breakpoint's."""
    mask = np.zeros((W, Fr), dtype=bool)
    for r in range(W):
        s = r if rows is None else int(rows[r])
        n = int(z["bp_n"][s]) if 0 <= s < len(z["clock"]) else 0
        if n == 0:
            mask[r] = True
            continue
        tau = np.float64(int(z["clock"][s]) + block - n_in) + np.arange(Fr, dtype=np.float64) * np.float64(hop)
        at = z["bp_t"][s, :n].astype(np.float64)
        mask[r] = (tau < at[0]) | (tau >= at[-1]) | np.isin(tau, at)
    return mask


def _assert_weights(got, want, exact, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, what
    ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    same_sign = np.signbit(got) == np.signbit(want)
    print(f"{what}: largest distance {int(ulp[same_sign].max())} ulp, exact in {float((ulp == 0).mean()):.3f} of the weights, "
          f"{int(exact.sum())} of {exact.size} frames owed exactly")
    assert (same_sign | ((got == 0) & (want == 0))).all() and ulp[same_sign].max() <= 1, what
    assert np.array_equal(got[exact], want[exact]), what


# ---- 1. the kernel against its statement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [512.0, 512 * 48000 / 44100], ids=["integral", "fractional"])
def test_kernel_matches_the_numpy_statement(ctx, dev, hop):
    """W = 5 rows over S = 4 slots, rows = [2, -1, 0, 4, 3] (-1 and 4 >= S are padding), K = 3, Fr = 37, P_max = 4.  Slot 0: three
    breakpoints - two frames of the window lie before the first, the second sits exactly on frame 5's time at hop 512, the last
    inside the window, so the frames behind it are held; slot 2: none (and a clock beyond 2^32); slot 3: one.  Slot 1 is not
    named."""
    W, S4, Fr, n_in, block = 5, 4, 37, 36 * 512, 4096
    rows = [2, -1, 0, 4, 3]
    z = glide_state(S4, P_MAX, K, seed=8)
    z["clock"][:] = [20000, 12345, 2 ** 33 + 7, 0]
    first = 20000 + block - n_in
    w0 = set_points(z, 0, [first + 2 * 512, first + 5 * 512, first + 30 * 512 + 100], 21)
    w3 = set_points(z, 3, [1000], 22)
    t = {k: torch.from_numpy(v).to(dev) for k, v in z.items()}
    out = torch.full((W, Fr, K), float("nan"), device=dev)
    got = ctx.bank_glide_(torch.tensor(rows, dtype=torch.int32).to(dev), t["clock"], t["bp_n"], t["bp_t"], t["bp_w"], t["spk_w"], out,
                          n_in, block, hop)
    torch.cuda.synchronize()
    ctx.poll_error()                                               # a padding row is no error
    assert got is out
    want, clock = glide_ref(rows, W, **z, Fr=Fr, n_in=n_in, block=block, hop=hop)
    got = out.cpu().numpy()
    exact = _exact_mask(rows, W, z, Fr, n_in, block, hop)
    _assert_weights(got, want, exact, f"hop {hop:.3f}")
    assert exact[[0, 1, 3, 4]].all() and exact[2, :2].all() and not exact[2, 6:27].any()
    pad = np.broadcast_to(np.array([1, 0, 0], dtype=np.float32), (Fr, K))
    assert np.array_equal(got[1], pad) and np.array_equal(got[3], pad)
    assert np.array_equal(got[0], np.broadcast_to(z["spk_w"][2], (Fr, K))) and np.array_equal(got[4], np.broadcast_to(w3[0], (Fr, K)))
    assert np.array_equal(got[2, :2], np.broadcast_to(w0[0], (2, K))) and np.array_equal(got[2, 31:], np.broadcast_to(w0[2], (6, K)))
    if hop == 512.0:
        assert exact[2, 2] and exact[2, 5] and np.array_equal(got[2, 2], w0[0]) and np.array_equal(got[2, 5], w0[1])
    assert (np.abs(np.diff(got[2, 2:28, 0])) > 0).all()             # the ramps do change from frame to frame
    # the clocks of slots 0, 2 and 3 moved by one block; slot 1's did not; nothing else of the state was written
    assert t["clock"].tolist() == clock.tolist() == [20000 + block, 12345, 2 ** 33 + 7 + block, block]
    for name in ("bp_n", "bp_t", "bp_w", "spk_w"):
        assert np.array_equal(t[name].cpu().numpy(), z[name]), name
    # rows = None: row r is slot r
    out4 = torch.full((S4, Fr, K), float("nan"), device=dev)
    t["clock"].copy_(torch.from_numpy(z["clock"]))
    ctx.bank_glide_(None, t["clock"], t["bp_n"], t["bp_t"], t["bp_w"], t["spk_w"], out4, n_in, block, hop)
    torch.cuda.synchronize()
    assert torch.equal(out4[[2, 0, 3]], out[[0, 2, 4]]) and t["clock"].tolist() == (z["clock"] + block).tolist()
    for bad in (dict(n_in=n_in, block=0, hop=hop), dict(n_in=n_in, block=block, hop=0.0)):
        with pytest.raises(ValueError):
            ctx.bank_glide_(None, t["clock"], t["bp_n"], t["bp_t"], t["bp_w"], t["spk_w"], out4, **bad)
    with pytest.raises(ValueError):
        ctx.bank_glide_(None, t["clock"].int(), t["bp_n"], t["bp_t"], t["bp_w"], t["spk_w"], out4, n_in, block, hop)


# ---- 2. a bank that could glide and does not ---------------------------------------------------------------------------------
def test_without_a_timeline_the_bank_is_the_bank_without_the_feature(dev, model):
    """Constant weights give the row mix's bits: emitted blocks and `last_signal` are equal bit for bit over 3 blocks, and
    `graph_builds` is equal."""
    glide, plain = _bank(model, dev, glide_breakpoints=P_MAX), _bank(model, dev)
    assert (glide.block, glide.n_in, glide.frames) == (4410, 22050, 44) and glide.graph is not None
    for s, mix in enumerate(MIXES):
        glide.set_speaker(s, spk_mix_dict=mix)
        plain.set_speaker(s, spk_mix_dict=mix)
    for k in range(3):
        x = _inputs(k, glide, dev)
        a, b = _push(glide, x), _push(plain, x)
        torch.cuda.synchronize()
        assert torch.equal(a, b), (k, float((a - b).abs().max()))
        assert torch.equal(glide.last_signal, plain.last_signal), k
        assert float(a.abs().max()) > 0 and float(glide.last_signal.abs().max()) > 1e-3
        assert torch.equal(glide.last_mix_w, glide.spk_w[:, None, :].expand(S, glide.frames, K)) and plain.last_mix_w is None
    assert glide.graph_builds == plain.graph_builds == 1
    assert glide.glide_clock.tolist() == [3 * glide.block] * S and not glide.glide_n.any()


# ---- 3. a timeline on one slot ---------------------------------------------------------------------------------------------
def test_timeline_on_one_slot_against_the_statement_and_the_eager_forward(dev, model):
    """Five blocks; slot 1 ramps from 0.15 s (inside block 2) to 0.35 s (before block 5).  Per block `last_mix_w` is the
    statement's and `last_signal` is the eager forward with `spk_mix_rows=(ids, last_mix_w)` and the gate, bit for bit; the graph
    and the eager bank agree bit for bit; `set_timeline` captures nothing."""
    import hipddsp
    graph, eager = _bank(model, dev, glide_breakpoints=P_MAX), _bank(model, dev, glide_breakpoints=P_MAX, use_graph=False)
    assert graph.graph_builds == 1 and eager.graph_builds == 0
    for bank in (graph, eager):
        for s, mix in enumerate(MIXES):
            bank.set_speaker(s, spk_mix_dict=mix)
        bank.set_timeline(1, SpeakerTimeline(RAMP))
    assert graph.graph_builds == 1 and graph.spk_ids.tolist() == [[2, 1, 1], [2, 5, 7], [7, 3, 4]]
    assert graph.glide_t[1].tolist() == [6615, 11025, 15435, 0] and graph.glide_n.tolist() == [0, 3, 0]
    ctx = hipddsp.context_for(dev)
    z = _state(graph)
    moving = 0
    for k in range(5):
        x = _inputs(k, graph, dev)
        a, b = _push(graph, x), _push(eager, x)
        torch.cuda.synchronize()
        want, z["clock"] = glide_ref(None, S, **z, Fr=graph.frames, n_in=graph.n_in, block=graph.block, hop=graph.hop_size)
        exact = _exact_mask(None, S, dict(z, clock=z["clock"] - graph.block), graph.frames, graph.n_in, graph.block, graph.hop_size)
        assert graph.last_mix_w.shape == (S, graph.frames, K)
        _assert_weights(graph.last_mix_w.cpu().numpy(), want, exact, f"block {k + 1}")
        assert graph.glide_clock.tolist() == z["clock"].tolist() == [(k + 1) * graph.block] * S
        moving += int((~exact[1]).sum())
        assert exact[0].all() and exact[2].all()
        # the graph and the eager bank: the same bits
        assert torch.equal(graph.last_mix_w, eager.last_mix_w), k
        assert torch.equal(a, b) and torch.equal(graph.last_signal, eager.last_signal), (k, float((a - b).abs().max()))
        # the signal is the eager per-frame forward on the block's own analysis, gated
        with torch.no_grad():
            sig = model(graph.last_units, graph.last_f0, graph.last_volume, None,
                        spk_mix_rows=(graph.spk_ids, graph.last_mix_w.clone()), noise=x["noise"])[0]
        ctx.volume_gate_(sig, graph.last_volume, THR, 512)
        torch.cuda.synchronize()
        assert torch.equal(graph.last_signal, sig), (k, float((graph.last_signal - sig).abs().max()))
        assert float(sig[1].abs().max()) > 1e-3
        if k == 0:                                                  # the whole window is older than the ramp: its first weights
            assert torch.equal(graph.last_mix_w[1], torch.tensor([1.0, 0, 0], device=dev).expand(graph.frames, K))
        if k == 4:                                                  # the newest frames lie behind the ramp: its last weights
            assert graph.last_mix_w[1, -1].tolist() == [0.0, np.float32(0.7), np.float32(0.3)]
            assert len({tuple(f) for f in graph.last_mix_w[1].tolist()}) > 10
    assert moving > 20 and graph.graph_builds == 1 and eager.graph_builds == 0


# ---- 4. a paused slot ---------------------------------------------------------------------------------------------------------
def test_a_paused_slot_keeps_its_clock_and_its_timeline(dev, model):
    """`active_widths=(1, 2)`; slot 2 glides and is named in calls 1 and 4 only.  Through calls 2 and 3 its rows of the glide
    state, of `spk_ids` and of the windows stay bit for bit, and call 4 gives it the weights of a bank in which it saw two calls."""
    tl = SpeakerTimeline([(0.0, 7), (0.3, {3: 0.5, 4: 0.5})])
    bank, other = (_bank(model, dev, glide_breakpoints=P_MAX, active_widths=(1, 2)) for _ in range(2))
    assert bank.graph_builds == other.graph_builds == 4
    for b in (bank, other):
        b.set_timeline(2, tl)
        b.set_timeline(0, SpeakerTimeline([(0.05, 1), (0.2, 2)]))
    kept = lambda: [t.clone() for t in (bank.glide_clock[2], bank.glide_n, bank.glide_t, bank.glide_w, bank.spk_ids[2], bank.windows[2])]  # noqa: E731
    calls = [[0, 2], [0, 1], [1], [1, 2]]
    for n, active in enumerate(calls):
        _push(bank, _inputs(n, bank, dev), active=active)
        torch.cuda.synchronize()
        assert bank.last_mix_w.shape == (len(active), bank.frames, K) and bank.last_active == tuple(active)
        if n == 0:
            after_first = kept()
            assert int(bank.glide_clock[2]) == bank.block and bank.windows[2].any()
        elif n < 3:
            for got, want in zip(kept(), after_first):
                assert torch.equal(got, want), n
    assert bank.glide_clock.tolist() == [2 * bank.block, 3 * bank.block, 2 * bank.block]
    x = _inputs(3, other, dev)
    _push(other, _inputs(0, other, dev), active=[0, 2])
    _push(other, x, active=[1, 2])
    torch.cuda.synchronize()
    assert torch.equal(bank.last_mix_w[1], other.last_mix_w[1])
    assert len({tuple(f) for f in bank.last_mix_w[1].tolist()}) > 5    # (a ramp, not a constant)
    assert torch.equal(bank.last_mix_w[0], torch.tensor([1.0, 0, 0], device=dev).expand(bank.frames, K))   # slot 1: no timeline
    assert bank.graph_builds == 4


# ---- 5. set_speaker and reset -------------------------------------------------------------------------------------------------
def test_set_speaker_ends_a_glide_and_reset_restarts_it(dev, model):
    bank = _bank(model, dev, glide_breakpoints=P_MAX)
    tl = SpeakerTimeline([(0.0, 2), (0.05, {2: 0.5, 5: 0.5}), (0.25, 5)])
    bank.set_timeline(0, tl)
    bank.set_timeline(1, tl)
    seen = []
    for k in range(2):
        _push(bank, _inputs(k, bank, dev))
        torch.cuda.synchronize()
        seen.append(bank.last_mix_w.clone())
    assert not torch.equal(seen[0][1], seen[1][1]) and len({tuple(f) for f in seen[1][0].tolist()}) > 5
    bank.set_speaker(0, spk_mix_dict={3: 0.25, 1: 0.75})
    bank.reset(1)
    assert bank.glide_n.tolist() == [0, 3, 0] and bank.glide_clock.tolist() == [2 * bank.block, 0, 2 * bank.block]
    _push(bank, _inputs(2, bank, dev))
    torch.cuda.synchronize()
    assert torch.equal(bank.last_mix_w[0], torch.tensor([0.25, 0.75, 0], device=dev).expand(bank.frames, K))   # constant from now on
    assert torch.equal(bank.last_mix_w[1], seen[0][1])                 # the glide of slot 1 started again from its beginning
    assert bank.glide_clock.tolist() == [3 * bank.block, bank.block, 3 * bank.block]
    assert bank.glide_t[1].tolist() == [0, 2205, 11025, 0] and bank.spk_ids[0].tolist() == [3, 1, 1] and bank.graph_builds == 1


# ---- 6. the raw-audio form: the launch inside the captured block ---------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_push_audio_glides_inside_the_captured_block(dev, model, crepe, encoder, use_graph):  # noqa: F811
    """`push_audio`: `ddsp_bank_glide` is part of `GraphedBlock`'s capture.  The capture's own runs leave the clocks where they
    were (0), a timeline set afterwards is followed without a new capture, and the weights are the statement's."""
    bank = _bank(model, dev, glide_breakpoints=P_MAX, use_graph=use_graph, units_encoder=encoder, f0_extractor="crepe",
                 crepe_ckpt=crepe, f0_dither=False)
    builds = bank.graph_builds
    assert builds == int(use_graph) and (bank.bank_graph is not None) == use_graph
    assert bank.glide_clock.tolist() == [0] * S and not bank.windows.any()
    bank.set_timeline(1, SpeakerTimeline([(0.0, 2), (0.15, {2: 0.5, 5: 0.5}), (0.3, 5)]))
    z = _state(bank)
    for k in range(2):
        x = _inputs(k, bank, dev)
        out = bank.push_audio(x["blocks"], noise=x["noise"])
        torch.cuda.synchronize()
        want, z["clock"] = glide_ref(None, S, **z, Fr=bank.frames, n_in=bank.n_in, block=bank.block, hop=bank.hop_size)
        exact = _exact_mask(None, S, dict(z, clock=z["clock"] - bank.block), bank.frames, bank.n_in, bank.block, bank.hop_size)
        _assert_weights(bank.last_mix_w.cpu().numpy(), want, exact, f"push_audio block {k + 1}")
        assert bank.glide_clock.tolist() == [(k + 1) * bank.block] * S and out.shape == (S, bank.block)
    assert len({tuple(f) for f in bank.last_mix_w[1].tolist()}) > 5 and bank.graph_builds == builds
