"""`realtime.StreamRenderer.push_audio`: the real-time block from the raw audio (window push, volume, CREPE f0, HuBERT-Soft
units, synthesis, gate - eager or as one HIP graph - then enhancer, resampling, splice) against the composition its caller had
to write before (eager `F0_Extractor.extract` + `Units_Encoder.encode` on a window of their own, then
`push_block(block, units=, f0=)`), bit for bit, and against the CPU chain of tests/test_gpu_stream_chain.py; the device-side
dither seed; `ddsp_stream_push`; a re-capture in the middle of a stream; refusals.

Weights are the deterministic fills of tests/crepe_cases.py ('tiny') and tests/hubert_cases.py."""
import numpy as np
import pytest
import torch

import crepe_cases as CC
import hubert_cases as HC
import synthetic
from conftest import rms
from test_gpu_stream_chain import RI, TIMING, _CpuChain, _enhancer

pytestmark = pytest.mark.gpu
BLOCKS = 8
PITCH = 2.0
THR, SPK = -45.0, 2


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


def _block(k, block, sr, rng):
    """Block k of the signal of tests/test_gpu_stream_chain.py: a 147 Hz tone plus noise, block 3 silent."""
    t = (np.arange(block) + k * block) / sr
    amp = 0.0 if k == 3 else 0.2
    return (amp * np.sin(2 * np.pi * 147.0 * t) + amp * 0.05 * rng.standard_normal(block)).astype(np.float32)


def _renderers(dev, crepe, encoder, timing, sr, use_graph, seed=43, enhancer=None, key="auto", **kw):
    """(the renderer under test, an analysis-free one with the same settings, the model's CPU state dict and config)."""
    import realtime
    block_time, xfade_time, buffer_num = TIMING[timing]
    model, cfg = synthetic.build_model("CombSub", seed=seed)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    common = dict(buffer_num=buffer_num, threshold_db=THR, spk_id=SPK, use_graph=use_graph, pitch_adjust=PITCH, enhancer=enhancer,
                  enhancer_adaptive_key=key)
    r = realtime.StreamRenderer(model, sr, block_time, xfade_time, dev, units_encoder=encoder, f0_extractor="crepe",
                                crepe_ckpt=crepe, **common, **kw)
    plain = realtime.StreamRenderer(model, sr, block_time, xfade_time, dev, **common)
    return r, plain, sd, cfg


def _eager_analysis(r, encoder, window, sr):
    """f0 (before the pitch shift) and units of `window` as a caller of the analysis-free renderer computes them."""
    f0 = r.f0_extractor.extract(window, uv_interp=True, silence_front=r.silence_front, dither=False)
    return f0[None, :, None], encoder.encode(window[None], sr, r.hop_size)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("sr", [44100, 48000])
@pytest.mark.parametrize("timing", ["config5", "gui"])
def test_push_audio_equals_composition_and_oracle(dev, crepe, encoder, timing, sr, use_graph):
    """Per block: `last_f0` / `last_units` equal the eager analysis of the test's own window, the emitted block and the SOLA
    shift equal those of `push_block(block, units=, f0=, noise=)` on an analysis-free renderer (all `torch.equal`), and the
    block is within 1e-4 RMS of the CPU chain fed the device's units and f0."""
    r, plain, sd, cfg = _renderers(dev, crepe, encoder, timing, sr, use_graph, f0_dither=False)
    assert r.frames == (87 if timing == "config5" else 388)
    assert r.f0_extractor.f0_min == 50.0 and r.f0_extractor.f0_max == 1100.0 and r.f0_extractor.sample_rate == sr
    cpu = _CpuChain(sd, cfg, r, sr, THR, SPK, None, PITCH, None, False)
    window = torch.zeros(r.n_in, device=dev)
    rng = np.random.Generator(np.random.PCG64(91))
    loudest = 0.0
    for k in range(BLOCKS):
        blk = _block(k, r.block, sr, rng)
        blk_d = torch.from_numpy(blk).to(dev)
        noise = synthetic.make_inputs(6000 + k, 1, r.frames)["noise"]
        window = torch.cat([window[r.block:], blk_d])
        f0, units = _eager_analysis(r, encoder, window, sr)
        em = r.push_audio(blk_d, noise=noise.to(dev))
        torch.cuda.synchronize()
        assert torch.equal(r.window, window), (k,)
        assert r.last_f0.shape == (1, r.frames, 1) and r.last_units.shape == (1, r.frames, 256) and r.last_volume.shape == (1, r.frames)
        assert torch.equal(r.last_f0, f0 * 2 ** (PITCH / 12)), (k, float((r.last_f0 - f0 * 2 ** (PITCH / 12)).abs().max()))
        assert torch.equal(r.last_units, units), (k, float((r.last_units - units).abs().max()))
        shift = int(r.splicer.last_shift.item())
        em_p = plain.push_block(blk_d, units=units, f0=f0, noise=noise.to(dev))
        torch.cuda.synchronize()
        assert em.shape == (r.block,)
        assert torch.equal(em, em_p), (k, float((em - em_p).abs().max()))
        assert shift == int(plain.splicer.last_shift.item())
        em_o, sh_o, _ = cpu.push(blk, {"units": units.cpu(), "f0": f0.cpu(), "noise": noise})
        d = rms(em.cpu() - em_o)
        print(f"{timing} {sr} graph={use_graph} block {k}: rms vs CPU chain {d:.3e} (block rms {rms(em_o):.3e}), shift {shift}/{sh_o}")
        assert shift == sh_o, (k, shift, sh_o)
        assert d < 1e-4, (k, d, rms(em_o))
        loudest = max(loudest, rms(em_o))
    assert loudest > 1e-3
    if use_graph:
        assert r.graph_builds == 1 and r.block_graph is not None


@pytest.mark.parametrize("timing,key", [("config5", 0), ("gui", "auto")])
def test_push_audio_with_enhancer_against_oracle(dev, crepe, encoder, tmp_path, timing, key):
    """The enhancer behind the captured block: 5e-4 max-abs against the CPU chain, equal keys and SOLA shifts."""
    enh = _enhancer(dev, tmp_path)
    r, _, sd, cfg = _renderers(dev, crepe, encoder, timing, 44100, True, enhancer=enh, key=key, f0_dither=False)
    cpu = _CpuChain(sd, cfg, r, 44100, THR, SPK, None, PITCH, key, False)
    window = torch.zeros(r.n_in, device=dev)
    rng = np.random.Generator(np.random.PCG64(91))
    loudest = 0.0
    for k in range(BLOCKS):
        blk = _block(k, r.block, 44100, rng)
        noise = synthetic.make_inputs(6000 + k, 1, r.frames)["noise"]
        blk_d = torch.from_numpy(blk).to(dev)
        window = torch.cat([window[r.block:], blk_d])
        f0, units = _eager_analysis(r, encoder, window, 44100)      # (the CPU chain applies the pitch shift itself)
        em = r.push_audio(blk_d, noise=noise.to(dev), rand_ini=RI)
        assert torch.equal(r.last_f0, f0 * 2 ** (PITCH / 12)) and torch.equal(r.last_units, units), (k,)
        em_o, sh_o, key_o = cpu.push(blk, {"units": units.cpu(), "f0": f0.cpu(), "noise": noise})
        d = float((em.cpu() - em_o).abs().max())
        print(f"{timing} key={key} block {k}: max abs vs CPU chain {d:.3e}, key {r.last_key}/{key_o}")
        assert int(r.splicer.last_shift.item()) == sh_o, (k,)
        assert r.last_key == key_o, (k, r.last_key, key_o)
        assert d < 5e-4, (k, d)
        loudest = max(loudest, rms(em_o))
    assert loudest > 1e-3


def test_dither_moves_between_replays(dev, crepe, encoder):
    """Under the graph the dither seed advances on the device: two replays over identical window content differ, and both
    stay within a bin's 20 cents of the undithered track."""
    r, _, _, _ = _renderers(dev, crepe, encoder, "config5", 44100, True, f0_dither=True)
    assert r.n_in == 5 * r.block
    rng = np.random.Generator(np.random.PCG64(7))
    t = np.arange(r.block) / 44100
    blk = torch.from_numpy((0.2 * np.sin(2 * np.pi * 150.0 * t) + 0.01 * rng.standard_normal(r.block)).astype(np.float32)).to(dev)
    tracks = []
    for k in range(7):                                   # from the fifth push on the window is five copies of the block
        r.push_audio(blk)
        if k >= 5:
            tracks.append(r.last_f0.clone())
    window = blk.repeat(5)
    assert torch.equal(r.window, window)
    plain = r.f0_extractor.extract(window, uv_interp=True, silence_front=r.silence_front, dither=False)[None, :, None] * 2 ** (PITCH / 12)
    torch.cuda.synchronize()
    assert float(plain.min()) > 1.5 * 50.0 * 2 ** (PITCH / 12)      # voiced frames (decoded bins), not the f0_min floor
    assert not torch.equal(tracks[0], tracks[1])
    for f0 in tracks:
        cents = 1200 * torch.log2(f0.double() / plain.double()).abs()
        assert float(cents.max()) <= 20.0 + 1e-2, float(cents.max())
        assert not torch.equal(f0, plain)


@pytest.mark.parametrize("case", ["sweep", "pair"])
def test_decode_dseed_equals_decode_and_advances(dev, ctx, crepe, case):
    import hipddsp
    probs = crepe.activations(CC.audio(case).to(dev))
    seed = 0x123456789ABCDEF0 >> 1
    want = ctx.crepe_decode(probs, 50.0, 1100.0, dither_seed=seed, dither=True, want_bins=True)
    word = torch.tensor([seed], dtype=torch.int64, device=dev)
    got = ctx.crepe_decode(probs, 50.0, 1100.0, dither=True, want_bins=True, seed_dev=word)
    again = ctx.crepe_decode(probs, 50.0, 1100.0, dither=True, seed_dev=word)
    torch.cuda.synchronize()
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    nxt = hipddsp.next_dither_seed(seed)
    assert not torch.equal(again[0], got[0])
    assert torch.equal(again[0], ctx.crepe_decode(probs, 50.0, 1100.0, dither_seed=nxt, dither=True)[0])
    assert int(word.item()) & ((1 << 64) - 1) == hipddsp.next_dither_seed(nxt) != seed
    with pytest.raises(ValueError):
        ctx.crepe_decode(probs, 50.0, 1100.0, dither=True, seed_dev=word.to(torch.int32))


@pytest.mark.parametrize("n_in,block", [(44100, 8820), (216000, 72000), (716, 715), (1000, 1)])
def test_stream_push_against_cat(dev, ctx, n_in, block):
    rng = np.random.Generator(np.random.PCG64(n_in + block))
    window = torch.from_numpy(rng.standard_normal(n_in).astype(np.float32)).to(dev)
    want = window.clone()
    ptr = window.data_ptr()
    for _ in range(5):
        blk = torch.from_numpy(rng.standard_normal(block).astype(np.float32)).to(dev)
        want = torch.cat([want[block:], blk])
        assert ctx.stream_push_(window, blk) is window
        torch.cuda.synchronize()
        assert window.data_ptr() == ptr and torch.equal(window, want)
    for bad in (n_in, n_in + 3, 0):
        with pytest.raises(ValueError):
            ctx.stream_push_(window, torch.ones(bad, device=dev))
    with pytest.raises(ValueError):
        ctx.stream_push_(window, window[:block])                  # the block may not lie inside the window
    torch.cuda.synchronize()
    assert torch.equal(window, want)


def test_recapture_keeps_the_stream(dev, crepe, encoder):
    """A new speaker mix between blocks 3 and 4 re-captures the whole-block graph: the window and the splicer's buffer are
    untouched by it, and the blocks after it equal the eager renderer's under the same switch."""
    import realtime
    model, _ = synthetic.build_model("CombSub", seed=47, device=dev)
    kw = dict(buffer_num=4, spk_id=3, units_encoder=encoder, f0_extractor="crepe", crepe_ckpt=crepe, f0_dither=False)
    rg = realtime.StreamRenderer(model, 44100, 0.2, 0.04, dev, use_graph=True, **kw)
    re = realtime.StreamRenderer(model, 44100, 0.2, 0.04, dev, use_graph=False, **kw)
    rng = np.random.Generator(np.random.PCG64(91))
    for k in range(BLOCKS):
        if k == 3:
            window, buf, graph_before = rg.window.clone(), rg.splicer.buffer.clone(), rg.block_graph
            for r in (rg, re):
                r.set_speaker(spk_mix_dict={1: 0.3, 3: 0.7})
            torch.cuda.synchronize()
            assert rg.block_graph is not graph_before and rg.graph_builds == 2 and re.graph_builds == 0
            assert torch.equal(rg.window, window) and torch.equal(rg.splicer.buffer, buf)
            assert float(window.abs().max()) > 0 and float(buf.abs().max()) > 0
        blk = torch.from_numpy(_block(k if k < 3 else k + 1, rg.block, 44100, rng)).to(dev)   # (no silent block here)
        noise = synthetic.make_inputs(7000 + k, 1, rg.frames)["noise"].to(dev)
        a, b = rg.push_audio(blk, noise=noise), re.push_block(blk, noise=noise)       # push_block without features: the same path
        torch.cuda.synchronize()
        assert torch.equal(a, b), (k, float((a - b).abs().max()))
        assert torch.equal(rg.window, re.window) and torch.equal(rg.last_f0, re.last_f0) and torch.equal(rg.last_units, re.last_units)
        assert float(a.abs().max()) > 0


def test_push_audio_refusals(dev, crepe, encoder):
    import realtime
    from ddsp.vocoder import F0_Extractor
    model, _ = synthetic.build_model("CombSub", seed=47, device=dev)
    args = (model, 48000, 0.2, 0.04, dev)
    hop = 512 * 48000 / 44100
    for bad in (F0_Extractor("crepe", 44100, hop, crepe_ckpt=crepe, device=dev),         # another rate
                F0_Extractor("crepe", 48000, 512, crepe_ckpt=crepe, device=dev)):        # another hop
        with pytest.raises(ValueError):
            realtime.StreamRenderer(*args, use_graph=False, units_encoder=encoder, f0_extractor=bad)
    with pytest.raises(ValueError):
        realtime.StreamRenderer(*args, use_graph=False, units_encoder=encoder)           # half an analysis
    r = realtime.StreamRenderer(*args, use_graph=False)
    with pytest.raises(ValueError):
        r.push_audio(torch.zeros(r.block, device=dev))                                   # no analysis configured
    good = F0_Extractor("crepe", 48000, hop, 50.0, 1100.0, crepe_ckpt=crepe, device=dev)
    r = realtime.StreamRenderer(*args, use_graph=False, units_encoder=encoder, f0_extractor=good)
    assert r.f0_extractor is good
    for n in (r.block - 1, r.block + 1):
        with pytest.raises(ValueError):
            r.push_audio(torch.zeros(n, device=dev))
    assert r.push_audio(torch.zeros(r.block, device=dev)).shape == (r.block,)
