"""`realtime.StreamBank(models=...)`: a bank whose slots each name one of M models.  The analysis of a call runs once over its
rows, then every model renders its own rows as a compact batch between the two row movers `ddsp_bank_features_gather` and
`ddsp_bank_signal_scatter`.  The movers alone against torch indexing; a two-model bank against single-model banks that run the
synthesiser at the same compact width, bit for bit; `set_model` between blocks; an uneven split and a model without rows; a call
with `active=`; the bank from raw audio; the shared enhancer stage.

Geometry: that of tests/test_gpu_bank_active.py ('config5': 0.2 s blocks, 87 frames at 44.1 kHz, S = 4 slots), injected noise and
source phases, 3 to 5 blocks.  Models: A = CombSub with one speaker, B = Sins with three (seeded random weights, the widths of
`synthetic.MODEL_CFG`)."""
import json

import numpy as np
import pytest
import torch

import crepe_cases as CC
import glue_cases as GC
import hubert_cases as HC
import synthetic
from conftest import rms
from test_bank_models_host import bank_model

pytestmark = pytest.mark.gpu
S, SR = 4, 44100
BLOCK_TIME, XFADE_TIME, BUFFER_NUM = 0.2, 0.04, 4          # 'config5'
THR = -45.0
TONES = (147.0, 220.0, 330.0, 196.0)
PITCHES = (0.0, 3.0, -2.0, 5.0)
KEYS = (2, "auto", 5, 0)
B_MIXES = {1: {2: 1.0}, 2: {3: 0.6, 1: 0.4}, 3: {1: 0.3, 3: 0.7}}     # the mix a slot sings with while it is on model B
MODES = ["block-graph", "block-eager", "audio-graph", "audio-eager", "block-graph-enhancer"]


@pytest.fixture(scope="module")
def models(dev, lib_path):
    return bank_model("CombSub", 1, 43, dev), bank_model("Sins", 3, 44, dev)


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


def _mode(how, crepe, encoder, enh):
    kw = dict(use_graph="graph" in how)
    if how.startswith("audio"):
        kw.update(units_encoder=encoder, f0_extractor="crepe", crepe_ckpt=crepe, f0_dither=False)
    if how.endswith("enhancer"):
        kw.update(enhancer=enh)
    return kw


def _dress(bank, slot, on_b):
    """Slot `slot` sings at its pitch and key, as speaker 1 of a model with one speaker or as its mix of model B."""
    if on_b:
        bank.set_speaker(slot, spk_mix_dict=B_MIXES[slot])
    bank.set_pitch(slot, PITCHES[slot])
    if bank.enhancer is not None:
        bank.set_enhancer_key(slot, KEYS[slot])


def _two(models, dev, on_b=(1, 3), **kw):
    """The two-model bank with the slots `on_b` on model B and the others on model A, every slot dressed."""
    bank = _bank(None, dev, models=list(models), **kw)
    for slot in range(S):
        if slot in on_b:
            bank.set_model(slot, 1)
        _dress(bank, slot, slot in on_b)
    return bank


def _one(model, dev, slots, on_b, **kw):
    """A single-model bank whose slots are dressed like those of the two-model bank: pitch and key everywhere, the mixes of
    model B on `slots` when the model is B."""
    bank = _bank(model, dev, **kw)
    for slot in range(S):
        _dress(bank, slot, on_b and slot in slots)
    return bank


def _inputs(k, bank, dev):
    """Step k of the four callers: blocks (4, block) of tones, units (4, Fr, 256), f0 (4, Fr, 1), noise (4, Fr * 512), phases (4, 9)."""
    rng = np.random.Generator(np.random.PCG64(500 + k))
    t = (np.arange(bank.block) + k * bank.block) / SR
    blocks = np.stack([0.2 * np.sin(2 * np.pi * f * t) + 0.01 * rng.standard_normal(bank.block) for f in TONES])
    z = synthetic.make_inputs(8000 + k, S, bank.frames)
    ri = torch.from_numpy(rng.uniform(0, 1, (S, 9)).astype(np.float32))
    return {"blocks": torch.from_numpy(blocks.astype(np.float32)).to(dev), "units": z["units"].to(dev), "f0": z["f0"].to(dev),
            "noise": z["noise"].to(dev), "rand_ini": ri.to(dev)}


def _push(bank, x, callers, active=None):
    """One call for the callers `callers` (their rows of the inputs, in this order)."""
    row = lambda name: x[name][list(callers)].contiguous()
    kw = {} if active is None else {"active": active}
    if bank.enhancer is not None:
        kw["rand_ini"] = row("rand_ini")
    if bank.f0_extractor is not None:
        return bank.push_audio(row("blocks"), noise=row("noise"), **kw)
    return bank.push_block(row("blocks"), row("units"), row("f0"), noise=row("noise"), **kw)


def _replays(bank):
    return [{W: chain.replays for W, chain in by_width.items()} for by_width in bank._model_rows]


# ---- 1. the row movers alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Fr,C,hop", [(8, 12, 16), (9, 12, 16), (9, 5, 3)], ids=["vectors", "odd-frames", "words"])
def test_row_movers_against_torch_indexing(ctx, dev, Fr, C, hop):
    """Fr = 8: every segment moves by 16-byte vectors; Fr = 9 with C = 12, hop = 16: the f0 and volume rows take the word path,
    units and noise the vectors; Fr = 9, C = 5, hop = 3: every segment by words."""
    R, K, T = 5, 3, Fr * hop
    g = torch.Generator().manual_seed(Fr * 100 + C)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)
    units, f0, volume, noise, w = rnd(R, Fr, C), rnd(R, Fr, 1), rnd(R, Fr), rnd(R, T), rnd(R, K)
    ids = torch.randint(1, 100, (R, K), generator=g).to(dev, torch.int32)
    batch = [t.clone() for t in (units, f0, volume, noise, ids, w)]

    def gather(table, with_noise=True):
        W = len(table)
        rows = torch.tensor(table, dtype=torch.int32).to(dev)
        c = dict(units=torch.full((W, Fr, C), 9.0, device=dev), f0=torch.full((W, Fr, 1), 9.0, device=dev),
                 volume=torch.full((W, Fr), 9.0, device=dev), noise=torch.full((W, T), 9.0, device=dev),
                 ids=torch.full((W, K), 9, dtype=torch.int32, device=dev), w=torch.full((W, K), 9.0, device=dev))
        out = ctx.bank_features_gather_(rows, units, f0, volume, (ids, w), c["units"], c["f0"], c["volume"], (c["ids"], c["w"]),
                                        *((noise, c["noise"]) if with_noise else ()))
        torch.cuda.synchronize()
        assert out is c["units"]
        return rows, c

    # (7 and -3 lie outside [0, R): padding rows like -1)
    table = [4, -1, 0, 7, 2, -3]
    real = [(r, s) for r, s in enumerate(table) if 0 <= s < R]
    rows, c = gather(table)
    idx = torch.tensor([s for _, s in real], device=dev)
    at = [r for r, _ in real]
    for name, src in (("units", units), ("f0", f0), ("volume", volume), ("noise", noise), ("ids", ids), ("w", w)):
        assert torch.equal(c[name][at], src.index_select(0, idx)), name
    for r in (1, 3, 5):
        assert not c["units"][r].any() and not c["f0"][r].any() and not c["volume"][r].any() and not c["noise"][r].any(), r
        assert c["ids"][r].tolist() == [1] * K and c["w"][r].tolist() == [1.0] + [0.0] * (K - 1), r
    _, c2 = gather(table, with_noise=False)                              # (no injected noise: that segment is left alone)
    assert torch.equal(c2["units"], c["units"]) and torch.equal(c2["f0"], c["f0"]) and torch.equal(c2["volume"], c["volume"])
    assert torch.equal(c2["ids"], c["ids"]) and torch.equal(c2["w"], c["w"]) and float(c2["noise"].min()) == 9.0
    for a, b in zip(batch, (units, f0, volume, noise, ids, w)):
        assert torch.equal(a, b)                                        # the batch is only read
    # the scatter: the named rows are written, the others keep the sentinel
    csig = rnd(len(table), T)
    sig = torch.full((R, T), -7.0, device=dev)
    assert ctx.bank_signal_scatter_(rows, csig, sig) is sig
    torch.cuda.synchronize()
    want = torch.full((R, T), -7.0, device=dev).index_copy_(0, idx, csig[at])
    assert torch.equal(sig, want) and float(sig[1].max()) == -7.0 == float(sig[3].min())
    # a table of padding alone writes nothing
    ctx.bank_signal_scatter_(torch.tensor([-1, R, 4096], dtype=torch.int32).to(dev), rnd(3, T), sig)
    torch.cuda.synchronize()
    assert torch.equal(sig, want)
    ctx.poll_error()                                                    # padding never sets the error word
    # refusals: tensors that overlap, a table of another length
    with pytest.raises(ValueError):
        ctx.bank_signal_scatter_(rows[:2], sig[:2], sig)
    with pytest.raises(ValueError):
        ctx.bank_signal_scatter_(rows[:3], csig, sig)
    with pytest.raises(ValueError):
        ctx.bank_features_gather_(rows[:2], units, f0, volume, (ids, w), units[:2], c["f0"][:2], c["volume"][:2],
                                  (c["ids"][:2], c["w"][:2]))
    torch.cuda.synchronize()
    assert torch.equal(sig, want)


# ---- 2. the synthesis stage, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", MODES)
def test_two_models_equal_their_single_model_banks(dev, models, crepe, encoder, enh, how):
    """Slots {0, 2} on A and {1, 3} on B: each pair is rendered at model width 2, as a single-model bank renders `active=` of
    that pair at compact width 2 - the same kernels on the same rows."""
    a, b = models
    kw = _mode(how, crepe, encoder, enh)
    builds = (1 + 2 * 3) if kw["use_graph"] else 0
    bank = _two(models, dev, **kw)
    ref_a, ref_b = _one(a, dev, (0, 2), False, active_widths=(2, 4), **kw), _one(b, dev, (1, 3), True, active_widths=(2, 4), **kw)
    assert bank.model_widths == (1, 2, 4) and bank.model_of_slot == [0, 1, 0, 1] and bank.graph_builds == builds
    for k in range(5):
        x = _inputs(k, bank, dev)
        got = _push(bank, x, range(S))
        for ref, pair in ((ref_a, [0, 2]), (ref_b, [1, 3])):
            want = _push(ref, x, pair, active=pair)
            torch.cuda.synchronize()
            d = float((got[pair] - want).abs().max())
            print(f"{how} block {k} slots {pair}: max |difference| to the single-model bank {d:.3e}, signal rms {rms(want):.3e}")
            assert torch.equal(got[pair], want), (k, pair, d)
            assert torch.equal(bank.last_signal[pair], ref.last_signal) and torch.equal(bank.last_shift[pair], ref.last_shift), (k, pair)
            assert torch.equal(bank.sola_buffer[pair], ref.sola_buffer[pair]) and torch.equal(bank.windows[pair], ref.windows[pair])
            if bank.enhancer is not None:
                assert torch.equal(bank.last_key[pair], ref.last_key), (k, pair)
        assert got.shape == (S, bank.block) and float(got[0].abs().max()) > 0 and float(got[1].abs().max()) > 0
        assert not torch.equal(got[0], got[2]) and not torch.equal(got[1], got[3])
    assert bank.graph_builds == builds
    assert _replays(bank) == [{1: 0, 2: 5, 4: 0}, {1: 0, 2: 5, 4: 0}]


# ---- 3. set_model between blocks --------------------------------------------------------------------------------------------
def test_set_model_between_blocks_captures_nothing(dev, models):
    """Slot 2 moves from A to B after block 2.  From then on the bank equals, bit for bit, a bank whose slot 2 was on B from the
    start and that took over the state rows (windows, SOLA buffers, speakers, pitches) at that block."""
    bank, ref = _two(models, dev), _two(models, dev, on_b=(1, 2, 3))
    builds = bank.graph_builds
    assert builds == 7
    for k in range(5):
        if k == 3:
            bank.set_model(2, 1, spk_mix_dict=B_MIXES[2])
            for name in ("windows", "sola_buffer", "spk_ids", "spk_w", "pitch"):
                getattr(ref, name).copy_(getattr(bank, name))
            assert bank.model_of_slot == ref.model_of_slot == [0, 1, 1, 1] and bank.graph_builds == builds
        x = _inputs(k, bank, dev)
        got, want = _push(bank, x, range(S)), _push(ref, x, range(S))
        torch.cuda.synchronize()
        if k >= 3:
            for slot in range(S):
                assert torch.equal(got[slot], want[slot]), (k, slot, float((got[slot] - want[slot]).abs().max()))
            assert torch.equal(bank.sola_buffer, ref.sola_buffer) and torch.equal(bank.windows, ref.windows), k
            assert torch.equal(bank.last_shift, ref.last_shift), k
        else:
            assert not torch.equal(got[2], want[2]), k                  # (A and B do not sing alike)
        assert float(got[2].abs().max()) > 0
    assert bank.graph_builds == builds
    assert _replays(bank) == [{1: 2, 2: 3, 4: 0}, {1: 0, 2: 3, 4: 2}]


# ---- 4. an uneven split, and a model without rows ---------------------------------------------------------------------------
def test_uneven_split_pads_and_an_idle_model_is_not_replayed(dev, models):
    a, _ = models
    bank = _two(models, dev, on_b=(3,))
    ref = _one(a, dev, (0, 1, 2), False, active_widths=(1, 2))
    for k in range(4):
        if k == 2:
            bank.set_model(3, 0)                                        # all four on A: B has no row from here on
        x = _inputs(k, bank, dev)
        got = _push(bank, x, range(S))
        want = _push(ref, x, (0, 1, 2), active=[0, 1, 2])               # (three rows at compact width 4, one padding row)
        torch.cuda.synchronize()
        assert torch.equal(got[:3], want), (k, float((got[:3] - want).abs().max()))
        assert float(got[3].abs().max()) > 0 and torch.isfinite(got).all()
    assert _replays(bank) == [{1: 0, 2: 0, 4: 4}, {1: 2, 2: 0, 4: 0}]
    assert bank._model_rows[0][4].named == (0, 1, 2, 3) and bank._model_rows[1][1].named == (3,)
    assert bank._model_rows[0][4].table.tolist() == [0, 1, 2, 3] and bank.graph_builds == 7


# ---- 5. with active= --------------------------------------------------------------------------------------------------------
def test_an_active_set_across_two_models(dev, models):
    """`active=[1, 2]` with slot 1 on B and slot 2 on A: each is one row at model width 1, as the single-model banks render it at
    compact width 1; the unnamed slots keep every state row."""
    a, b = models
    bank = _two(models, dev, active_widths=(1, 2))
    ref_a, ref_b = _one(a, dev, (2,), False, active_widths=(1, 2)), _one(b, dev, (1,), True, active_widths=(1, 2))
    assert bank.graph_builds == 4 + 6                                   # (full width and the ladder 1, 2, 4; two models by three widths)
    pattern = torch.arange(bank.n_in, device=dev, dtype=torch.float32) * 1e-4 + 0.5
    bank.windows[0], bank.windows[3] = pattern, -pattern
    bank.sola_buffer[0], bank.sola_buffer[3] = pattern[:bank.xfade] + 1, pattern[:bank.xfade] - 2
    state = lambda: [t[[0, 3]].clone() for t in (bank.windows, bank.sola_buffer, bank.spk_ids, bank.spk_w, bank.pitch)]
    before = state()
    for k in range(3):
        x = _inputs(k, bank, dev)
        got = _push(bank, x, (1, 2), active=[1, 2])
        want_b, want_a = _push(ref_b, x, (1,), active=[1]), _push(ref_a, x, (2,), active=[2])
        torch.cuda.synchronize()
        assert got.shape == (2, bank.block) and bank.last_active == (1, 2) and bank.last_signal.shape[0] == 2
        assert torch.equal(got[0], want_b[0]), (k, float((got[0] - want_b[0]).abs().max()))
        assert torch.equal(got[1], want_a[0]), (k, float((got[1] - want_a[0]).abs().max()))
        assert torch.equal(bank.sola_buffer[1], ref_b.sola_buffer[1]) and torch.equal(bank.sola_buffer[2], ref_a.sola_buffer[2]), k
        for name, p, q in zip(("windows", "sola_buffer", "spk_ids", "spk_w", "pitch"), before, state()):
            assert torch.equal(p, q), (k, name)
        assert float(got[0].abs().max()) > 0 and float(got[1].abs().max()) > 0
    assert _replays(bank) == [{1: 3, 2: 0, 4: 0}, {1: 3, 2: 0, 4: 0}] and bank.graph_builds == 10
    assert bank._model_rows[0][1].named == (1,) and bank._model_rows[1][1].named == (0,)    # rows of the CALL, not slots


# ---- 6. from raw audio ------------------------------------------------------------------------------------------------------
def test_push_audio_shares_one_analysis(dev, models, crepe, encoder):
    """The analysis is the single-model bank's graph body at the same width: units, f0 and volume bit for bit.  Every slot's
    signal before the splice against the single-model bank of its own model (rendered there at width 4, here at width 2): the
    bound tests/test_gpu_stream_bank.py holds a bank row to a solo renderer to, 1e-4 in RMS."""
    a, b = models
    kw = _mode("audio-graph", crepe, encoder, None)
    bank = _two(models, dev, **kw)
    refs = {0: _one(a, dev, (0, 2), False, **kw), 1: _one(b, dev, (1, 3), True, **kw)}
    assert bank.graph_builds == 7 and bank.bank_graph is not None and bank.bank_graph.sig is None
    loudest = 0.0
    for k in range(4):
        x = _inputs(k, bank, dev)
        got = _push(bank, x, range(S))
        assert got.shape == (S, bank.block)
        for ref in refs.values():
            _push(ref, x, range(S))
        torch.cuda.synchronize()
        for name in ("last_units", "last_f0", "last_volume"):
            assert torch.equal(getattr(bank, name), getattr(refs[0], name)), (k, name)
        assert torch.equal(bank.last_units, refs[1].last_units) and torch.equal(bank.last_volume, refs[1].last_volume), k
        assert torch.equal(bank.windows, refs[0].windows), k
        for slot in range(S):
            want = refs[bank.model_of_slot[slot]].last_signal[slot]
            d = rms(bank.last_signal[slot] - want)
            print(f"block {k} slot {slot}: signal rms vs its own model's bank {d:.3e} (signal rms {rms(want):.3e})")
            assert d < 1e-4, (k, slot, d)
            loudest = max(loudest, rms(want))
    assert loudest > 1e-3 and bank.graph_builds == 7


# ---- 7. the shared enhancer -------------------------------------------------------------------------------------------------
def test_the_enhancer_stage_is_shared(dev, models, enh):
    """The layout of test 2 through one enhancer: its input rows are the gated signals of the single-model banks (at 44.1 kHz
    their `last_signal` is the gated signal itself), every row has its own key, the output is finite and a block long."""
    import realtime
    a, b = models
    bank = _two(models, dev, enhancer=enh)
    ref_a, ref_b = _one(a, dev, (0, 2), False, active_widths=(2, 4)), _one(b, dev, (1, 3), True, active_widths=(2, 4))
    cut = realtime.key_cut_frames(bank.silence_front, SR, 512)
    for k in range(3):
        x = _inputs(k, bank, dev)
        got = _push(bank, x, range(S))
        for ref, pair in ((ref_a, [0, 2]), (ref_b, [1, 3])):
            _push(ref, x, pair, active=pair)
            torch.cuda.synchronize()
            assert torch.equal(bank.enhancer_graph.sig[pair], ref.last_signal), (k, pair)
        assert got.shape == (S, bank.block) and torch.isfinite(got).all() and float(got.abs().max()) > 0
        assert bank.last_signal.shape == (S, bank.block + bank.xfade + bank.search + bank.delay)
        keys = bank.last_key.tolist()
        auto = min(12, realtime.auto_key(float(bank.last_f0[1, cut:].max())))
        assert keys == [2, auto, 5, 0], (k, keys, auto)
    assert bank.graph_builds == 7
