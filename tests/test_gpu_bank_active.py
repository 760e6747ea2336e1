"""Active sets of `realtime.StreamBank`: a call that names its slots advances only them, as a compact batch from a ladder of
pre-captured widths.  A compact batch against an ordinary bank of that width bit for bit (same kernels, same shapes), padding
rows, paused slots, a caller that rejoins, set changes without a capture, one row against the solo chain, and the row mover
`ddsp_bank_gather` / `ddsp_bank_scatter` alone against index arithmetic.

Geometry: that of tests/test_gpu_stream_bank.py ('config5': 0.2 s blocks, 87 frames at 44.1 kHz) with S = 4 slots and
`active_widths=(1, 2)`, so the ladder is 1, 2, 4; injected noise and source phases; 3 to 8 blocks."""
import json

import numpy as np
import pytest
import torch

import crepe_cases as CC
import glue_cases as GC
import hubert_cases as HC
import synthetic
from conftest import rms

pytestmark = pytest.mark.gpu
S, SR = 4, 44100
BLOCK_TIME, XFADE_TIME, BUFFER_NUM = 0.2, 0.04, 4          # 'config5'
THR = -45.0
TONES = (147.0, 220.0, 330.0, 196.0)
MIXES = [{2: 1.0}, {1: 0.3, 5: 0.7}, {7: 0.5, 3: 0.25, 4: 0.25}, {9: 0.6, 2: 0.4}]
PITCHES = (0.0, 3.0, -2.0, 5.0)
KEYS = (2, "auto", 5, 0)


@pytest.fixture(scope="module")
def model(dev, lib_path):
    return synthetic.build_model("CombSub", seed=43, device=dev)[0]


@pytest.fixture(scope="module")
def crepe(dev, lib_path):
    from ddsp.crepe import Crepe
    m = Crepe("tiny")
    m.load_state_dict(CC.fill("tiny"))
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def encoder(dev, lib_path, tmp_path_factory):
    from ddsp.hubert import HubertSoft
    from ddsp.vocoder import Units_Encoder
    path = str(tmp_path_factory.mktemp("hubert") / "hubert-soft.pt")
    torch.save(HC.fill({k: tuple(v.shape) for k, v in HubertSoft().state_dict().items()}), path)
    return Units_Encoder("hubertsoft", path, device=dev)


@pytest.fixture(scope="module")
def enh(dev, lib_path, tmp_path_factory):
    """The narrow synthetic generator of tests/test_gpu_stream_bank_enhancer.py."""
    from enhancer import Enhancer
    tmp = tmp_path_factory.mktemp("nsf")
    with open(tmp / "config.json", "w") as fh:
        json.dump(dict(GC.NSF_CONFIG), fh)
    torch.save({"generator": GC.nsf_state_dict()}, tmp / "model")
    return Enhancer("nsf-hifigan", str(tmp / "model"), device=dev)


def _bank(model, dev, n=S, **kw):
    import realtime
    return realtime.StreamBank(model, n, SR, BLOCK_TIME, XFADE_TIME, dev, buffer_num=BUFFER_NUM, threshold_db=THR, **kw)


def _dress(bank, slot, like):
    """Slot `slot` of `bank` sings as caller `like` (mix, pitch and, with an enhancer, key request)."""
    bank.set_speaker(slot, spk_mix_dict=MIXES[like])
    bank.set_pitch(slot, PITCHES[like])
    if bank.enhancer is not None:
        bank.set_enhancer_key(slot, KEYS[like])


def _inputs(k, bank, dev):
    """Step k of the four callers: blocks (4, block) of tones, units (4, Fr, 256), f0 (4, Fr, 1), noise (4, Fr * 512), phases (4, 9)."""
    rng = np.random.Generator(np.random.PCG64(500 + k))
    t = (np.arange(bank.block) + k * bank.block) / SR
    blocks = np.stack([0.2 * np.sin(2 * np.pi * f * t) + 0.01 * rng.standard_normal(bank.block) for f in TONES])
    z = synthetic.make_inputs(8000 + k, S, bank.frames)
    ri = torch.from_numpy(rng.uniform(0, 1, (S, 9)).astype(np.float32))
    return {"blocks": torch.from_numpy(blocks.astype(np.float32)).to(dev), "units": z["units"].to(dev), "f0": z["f0"].to(dev),
            "noise": z["noise"].to(dev), "rand_ini": ri.to(dev)}


def _push(bank, x, callers, active=None, audio=False):
    """One call for the callers `callers` (their rows of the inputs, in this order)."""
    row = lambda name: x[name][list(callers)].contiguous()
    kw = {} if active is None else {"active": active}
    if bank.enhancer is not None:
        kw["rand_ini"] = row("rand_ini")
    if audio:
        return bank.push_audio(row("blocks"), noise=row("noise"), **kw)
    return bank.push_block(row("blocks"), row("units"), row("f0"), noise=row("noise"), **kw)


# ---- 1. same kernels, same shapes: bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["block-graph", "block-eager", "audio-graph", "audio-eager", "block-graph-enhancer"])
def test_width_2_equals_a_bank_of_2(dev, model, crepe, encoder, enh, how):
    audio, use_graph = how.startswith("audio"), "graph" in how
    kw = dict(use_graph=use_graph)
    if audio:
        kw.update(units_encoder=encoder, f0_extractor="crepe", crepe_ckpt=crepe, f0_dither=False)
    if how.endswith("enhancer"):
        kw.update(enhancer=enh)
    bank, ref = _bank(model, dev, active_widths=(1, 2), **kw), _bank(model, dev, n=2, **kw)
    assert bank.active_widths == (1, 2, 4) and bank.graph_builds == (4 if use_graph else 0) and ref.graph_builds == int(use_graph)
    for slot in range(S):
        _dress(bank, slot, slot)
    _dress(ref, 0, 1)
    _dress(ref, 1, 3)
    for k in range(3):
        x = _inputs(k, bank, dev)
        got = _push(bank, x, (1, 3), active=[1, 3], audio=audio)
        want = _push(ref, x, (1, 3), audio=audio)
        torch.cuda.synchronize()
        assert got.shape == (2, bank.block) and bank.last_active == (1, 3) and ref.last_active is None
        assert torch.equal(got, want), (k, float((got - want).abs().max()))
        assert torch.equal(bank.last_f0, ref.last_f0) and torch.equal(bank.last_shift, ref.last_shift), k
        assert bank.last_f0.shape == (2, bank.frames, 1) and bank.last_shift.shape == (2,)
        assert bank.last_units.shape[:2] == bank.last_volume.shape == (2, bank.frames) and bank.last_signal.shape[0] == 2
        assert torch.equal(bank.sola_buffer[[1, 3]], ref.sola_buffer), k
        assert torch.equal(bank.windows[[1, 3]], ref.windows), k
        assert not bank.windows[[0, 2]].any() and not bank.sola_buffer[[0, 2]].any()
        if bank.enhancer is not None:
            assert torch.equal(bank.last_key, ref.last_key) and bank.last_key.shape == (2,)
            assert int(bank.last_key[1]) == 0                       # (slot 3's fixed request went along)
        assert float(got[0].abs().max()) > 0 and not torch.equal(got[0], got[1])
    assert bank.graph_builds == (4 if use_graph else 0)


# ---- 2. padding -------------------------------------------------------------------------------------------------------------
def test_three_rows_at_width_4_pad_one(dev, model):
    bank, ref = _bank(model, dev, active_widths=(1, 2)), _bank(model, dev)
    for slot in range(S):
        _dress(bank, slot, slot)
    for r, caller in enumerate((0, 2, 3)):
        _dress(ref, r, caller)
    ref.set_speaker(3, spk_id=1)
    ref.set_pitch(3, 0.0)
    for k in range(3):
        x = _inputs(k, bank, dev)
        got = _push(bank, x, (0, 2, 3), active=[0, 2, 3])
        y = {n: v[[0, 2, 3, 1]].contiguous() for n, v in x.items()}
        y["blocks"][3] = 0
        y["units"][3] = 0
        want = _push(ref, y, (0, 1, 2, 3))
        torch.cuda.synchronize()
        assert got.shape == (3, bank.block) and bank.last_shift.shape == (3,) and bank.last_signal.shape[0] == 3
        assert torch.equal(got, want[:3]), (k, float((got - want[:3]).abs().max()))
        assert torch.equal(bank.last_shift, ref.last_shift[:3]) and torch.equal(bank.last_f0, ref.last_f0[:3])
        assert torch.equal(bank.sola_buffer[[0, 2, 3]], ref.sola_buffer[:3]) and not bank.sola_buffer[1].any()
        assert float(got.abs().max()) > 0


# ---- 3. paused means untouched ----------------------------------------------------------------------------------------------
def test_paused_slots_are_untouched(dev, model, enh):
    bank = _bank(model, dev, active_widths=(1, 2), enhancer=enh)
    for slot in range(S):
        _dress(bank, slot, slot)
    pattern = torch.arange(bank.n_in, device=dev, dtype=torch.float32) * 1e-4 + 0.5
    bank.windows[0], bank.windows[2] = pattern, -pattern
    bank.sola_buffer[0], bank.sola_buffer[2] = pattern[:bank.xfade] + 1, pattern[:bank.xfade] - 2
    state = lambda: [t[[0, 2]].clone() for t in (bank.windows, bank.sola_buffer, bank.spk_ids, bank.spk_w, bank.pitch, bank.enhancer_request)]
    before = state()
    assert before[2].tolist() == [[2, 1, 1, 1], [7, 3, 4, 1]] and before[5].tolist() == [2, 5]
    for k in range(3):
        got = _push(bank, _inputs(k, bank, dev), (1, 3), active=[1, 3])
        torch.cuda.synchronize()
        for name, a, b in zip(("windows", "sola_buffer", "spk_ids", "spk_w", "pitch", "enhancer_request"), before, state()):
            assert torch.equal(a, b), (k, name)
        assert float(got.abs().max()) > 0 and bank.windows[1].any() and bank.sola_buffer[3].any()


# ---- 4. rejoin --------------------------------------------------------------------------------------------------------------
def test_a_caller_that_rejoins_carries_on(dev, model):
    """Slot 2 is active in blocks 0-1, paused in 2-3 and active in 4-5 (slot 0 in every block): its four emitted blocks are
    those of row 1 of a 2-slot bank that was pushed the same four steps back to back."""
    bank, ref = _bank(model, dev, active_widths=(1, 2)), _bank(model, dev, n=2)
    _dress(bank, 0, 0)
    _dress(bank, 2, 2)
    _dress(ref, 0, 0)
    _dress(ref, 1, 2)
    step = 0
    for k in range(6):
        x = _inputs(k, bank, dev)
        if k in (2, 3):
            got = _push(bank, x, (0,), active=[0])
            assert got.shape == (1, bank.block) and bank.last_active == (0,)
            continue
        y = _inputs(step, bank, dev)                                  # slot 2's caller is at its own step
        x = {n: torch.stack([x[n][0], y[n][2]]) for n in x}
        got = _push(bank, x, (0, 1), active=[0, 2])
        want = _push(ref, x, (0, 1))
        torch.cuda.synchronize()
        assert torch.equal(got[1], want[1]), (k, float((got[1] - want[1]).abs().max()))
        assert torch.equal(bank.windows[2], ref.windows[1]) and torch.equal(bank.sola_buffer[2], ref.sola_buffer[1]), k
        assert int(bank.last_shift[1]) == int(ref.last_shift[1]) and float(got[1].abs().max()) > 0
        step += 1
    assert step == 4 and bank.graph_builds == 4


# ---- 5. changing the set captures nothing -----------------------------------------------------------------------------------
def test_changing_the_set_captures_nothing(dev, model, enh):
    bank = _bank(model, dev, active_widths=(1, 2), enhancer=enh)
    assert bank.graph_builds == 4

    def addresses():
        held = [bank.windows, bank.sola_buffer, bank.spk_ids, bank.spk_w, bank.pitch, bank.enhancer_request]
        for rows in [bank._full, *bank._compact.values()]:
            held += [rows.windows, rows.splicer.buffer, rows.spk_ids, rows.spk_w, rows.pitch, rows.request]
            held += [] if rows.rows is None else [rows.rows]
            held += [rows.graph.units, rows.graph.f0, rows.graph.volume, rows.graph.noise, rows.graph.out[0]]
            held += [rows.enhancer_graph.sig, rows.enhancer_graph.f0, rows.enhancer_graph.rand_ini, rows.enhancer_graph.tail]
        return [t.data_ptr() for t in held], [id(r.graph.graph) for r in [bank._full, *bank._compact.values()]]

    before = addresses()
    assert len(set(before[0])) == len(before[0]) - 6                  # (the full rows ARE the bank's state)
    for k, active in enumerate([[2], [0, 3], [0, 1, 3], None, [1], [1, 2], [1, 2, 3], None]):
        callers = range(S) if active is None else active
        got = _push(bank, _inputs(k, bank, dev), callers, active=active)
        torch.cuda.synchronize()
        assert got.shape == (len(callers), bank.block) and float(got.abs().max()) > 0
        assert bank.last_active == (None if active is None else tuple(active)) and bank.last_key.shape == (len(callers),)
        assert bank.graph_builds == 4 and addresses() == before, k


# ---- 6. against the solo chain ----------------------------------------------------------------------------------------------
def test_one_active_row_against_the_solo_renderer(dev, model):
    """As test_bank_against_solo_renderers of tests/test_gpu_stream_bank.py, with its bound: the signal before the splice in RMS
    (< 1e-4), the splice itself bit for bit on the bank's own signal."""
    import realtime
    bank = _bank(model, dev, active_widths=(1, 2))
    bank.set_speaker(2, spk_mix_dict=MIXES[1])
    bank.set_pitch(2, 2.0)
    solo = realtime.StreamRenderer(model, SR, BLOCK_TIME, XFADE_TIME, dev, buffer_num=BUFFER_NUM, threshold_db=THR, use_graph=False,
                                   pitch_adjust=2.0, spk_mix_dict=MIXES[1])
    push, seen = solo.splicer.push, []
    solo.splicer.push = lambda audio: (seen.append(audio.clone()), push(audio))[1]
    splicer = realtime.Splicer(SR, BLOCK_TIME, XFADE_TIME, dev)
    assert (bank.n_in, bank.frames, bank.block) == (solo.n_in, solo.frames, solo.block)
    loudest = 0.0
    for k in range(4):
        x = _inputs(k, bank, dev)
        got = _push(bank, x, (2,), active=[2])
        solo.push_block(x["blocks"][2], units=x["units"][2:3], f0=x["f0"][2:3], noise=x["noise"][2:3])
        torch.cuda.synchronize()
        want = seen[-1]
        assert bank.last_signal.shape == (1, want.numel())
        d = rms(bank.last_signal[0] - want)
        print(f"block {k}: signal rms vs the solo renderer {d:.3e} (signal rms {rms(want):.3e})")
        assert d < 1e-4, (k, d)
        e = splicer.push(bank.last_signal[0].contiguous())
        assert torch.equal(got[0], e) and int(bank.last_shift[0]) == int(splicer.last_shift), k
        loudest = max(loudest, rms(want))
    assert loudest > 1e-3


# ---- 7. the row movers alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,block", [(1000, 37), (1024, 64)], ids=["words", "vectors"])
def test_bank_gather_and_scatter_against_index_arithmetic(ctx, dev, n_in, block):
    n, K, xfade = 5, 3, 52 if block == 64 else 51
    g = torch.Generator().manual_seed(n_in)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)
    windows, sola, pitch, w = rnd(n, n_in), rnd(n, xfade), rnd(n), rnd(n, K)
    ids = torch.randint(1, 100, (n, K), generator=g).to(dev, torch.int32)
    request = torch.randint(-1, 12, (n,), generator=g).to(dev, torch.int32)
    state = lambda: [t.clone() for t in (windows, sola, ids, w, pitch, request)]

    def gather(table):
        W = len(table)
        rows = torch.tensor(table, dtype=torch.int32).to(dev)
        blocks = rnd(W, block)
        c = dict(cwindows=torch.full((W, n_in), 9.0, device=dev), csola=torch.full((W, xfade), 9.0, device=dev),
                 cids=torch.full((W, K), 9, dtype=torch.int32, device=dev), cw=torch.full((W, K), 9.0, device=dev),
                 cpitch=torch.full((W,), 9.0, device=dev), creq=torch.full((W,), 9, dtype=torch.int32, device=dev))
        out = ctx.bank_gather_(rows, blocks, windows, c["cwindows"], sola, c["csola"], (ids, w), (c["cids"], c["cw"]), pitch,
                               c["cpitch"], request, c["creq"])
        torch.cuda.synchronize()
        assert out is c["cwindows"]
        return rows, blocks, c

    before = state()
    rows, blocks, c = gather([4, -1, 0])
    want = before[0].clone()
    for r, s in ((0, 4), (2, 0)):
        want[s] = torch.cat([before[0][s, block:], blocks[r]])
        assert torch.equal(c["cwindows"][r], want[s]) and torch.equal(c["csola"][r], sola[s])
        assert torch.equal(c["cids"][r], ids[s]) and torch.equal(c["cw"][r], w[s])
        assert torch.equal(c["cpitch"][r], pitch[s]) and torch.equal(c["creq"][r], request[s])
    assert torch.equal(windows, want)                                   # slots 1, 2, 3 as they were; 0 and 4 pushed in place
    assert not c["cwindows"][1].any() and not c["csola"][1].any() and c["cids"][1].tolist() == [1] * K
    assert c["cw"][1].tolist() == [1.0] + [0.0] * (K - 1) and float(c["cpitch"][1]) == 1.0 and int(c["creq"][1]) == 0
    for a, b in zip(before[1:], state()[1:]):
        assert torch.equal(a, b)
    # the spliced buffers go back to slots 4 and 0 alone
    spliced = rnd(3, xfade)
    assert ctx.bank_scatter_(rows, spliced, sola) is sola
    torch.cuda.synchronize()
    want_sola = before[1].clone()
    want_sola[4], want_sola[0] = spliced[0], spliced[2]
    assert torch.equal(sola, want_sola)
    # an entry outside [0, S) is a padding row: nothing of any slot is written
    before = state()
    rows, _, c = gather([7])
    assert not c["cwindows"].any() and not c["csola"].any() and float(c["cpitch"][0]) == 1.0 and int(c["creq"][0]) == 0
    ctx.bank_scatter_(rows, rnd(1, xfade), sola)
    torch.cuda.synchronize()
    for a, b in zip(before, state()):
        assert torch.equal(a, b)
    # refusals: W > S, block >= n_in
    with pytest.raises(ValueError):
        gather([0, 1, 2, 3, 4, -1])
    with pytest.raises(ValueError):
        ctx.bank_gather_(rows, rnd(1, n_in), windows, c["cwindows"], sola, c["csola"], (ids, w), (c["cids"], c["cw"]), pitch,
                         c["cpitch"], request, c["creq"])
    with pytest.raises(ValueError):
        ctx.bank_scatter_(torch.zeros(6, dtype=torch.int32, device=dev), rnd(6, xfade), sola)
    torch.cuda.synchronize()
    for a, b in zip(before, state()):
        assert torch.equal(a, b)
