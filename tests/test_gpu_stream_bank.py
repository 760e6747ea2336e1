"""`realtime.StreamBank`: S streams of one geometry advanced by one block per call - the batched glue kernels against the solo
ones bit for bit, the per-row speaker mix of the control network against rows rendered alone, speaker / pitch changes
without a new capture, the bank against solo renderers, `push_audio` against its composition, isolation of the rows, refusals.

S = 3 (a wrong row index shows at rows 1 and 2), the 'config5' timing (0.2 s blocks, 87 frames at 44.1 kHz), 6 blocks, a tone of
its own in every row (147, 220, 330 Hz plus 5 % noise), row 1 silent in block 3.  Weights: `synthetic.build_model('CombSub')`,
the 'tiny' CREPE fill of tests/crepe_cases.py and the HuBERT fill of tests/hubert_cases.py."""
import numpy as np
import pytest
import torch

import crepe_cases as CC
import hubert_cases as HC
import synthetic
from conftest import rms
from oracle import realtime as RT

pytestmark = pytest.mark.gpu
S, BLOCKS = 3, 6
BLOCK_TIME, XFADE_TIME, BUFFER_NUM = 0.2, 0.04, 4          # 'config5'
TONES = (147.0, 220.0, 330.0)
THR = -45.0
MIXES = [{2: 1.0}, {1: 0.3, 5: 0.7}, {7: 0.5, 3: 0.25, 4: 0.25}]


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
def model(dev, lib_path):
    return synthetic.build_model("CombSub", seed=43, device=dev)[0]


def _blocks(k, block, sr, rng, silent=((1, 3),)):
    """Block k of the three streams (S, block): row s a TONES[s] tone plus 5 % noise; row 1 is silent in block 3."""
    t = (np.arange(block) + k * block) / sr
    rows = []
    for s, f in enumerate(TONES):
        amp = 0.0 if (s, k) in silent else 0.2
        rows.append(amp * np.sin(2 * np.pi * f * t) + amp * 0.05 * rng.standard_normal(block))
    return torch.from_numpy(np.stack(rows).astype(np.float32))


def _frames_inputs(k, frames, dev):
    """units (S, Fr, 256), f0 (S, Fr, 1) and noise (S, Fr * 512) of block k for the analysis-free calls."""
    z = synthetic.make_inputs(8000 + k, S, frames)
    return z["units"].to(dev), z["f0"].to(dev), z["noise"].to(dev)


def _bank(model, sr, dev, **kw):
    import realtime
    return realtime.StreamBank(model, S, sr, BLOCK_TIME, XFADE_TIME, dev, buffer_num=BUFFER_NUM, threshold_db=THR, **kw)


# ---- 1. the batched glue equals the solo kernels ---------------------------------------------------------------------------
def test_sola_batch_equals_solo_and_oracle(ctx, dev):
    """Step 0: rows are copies of one noisy tone delayed by 0, 57 and 211 samples and the buffer is a piece of row 0 at lag
    100, so the shifts are 100, 157 and 311 (and the three tails handed over are one piece of audio).  Step 1: the same tone
    at a phase and with a noise draw of each row's own, so that the buffers step 2 would start from differ per row."""
    block, xfade, search, delay = 8820, 1764, 441, 882
    n_audio = 87 * 512
    rng = np.random.Generator(np.random.PCG64(17))
    delays = (0, 57, 211)
    bufs = None
    for step in range(2):
        t = np.arange(n_audio + 211) / 44100
        base = (0.2 * np.sin(2 * np.pi * 147.0 * t + step) + 0.01 * rng.standard_normal(t.size)).astype(np.float32)
        audio = torch.from_numpy(np.stack([base[211 - d:211 - d + n_audio] for d in delays]))
        if step == 1:
            own = [0.2 * np.sin(2 * np.pi * 147.0 * t[:n_audio] + 1.3 * s) + 0.01 * rng.standard_normal(n_audio) for s in range(S)]
            audio = torch.from_numpy(np.stack(own).astype(np.float32))
        if bufs is None:
            x0 = audio[0, n_audio - block - xfade - search - delay:]
            bufs = x0[100:100 + xfade].repeat(S, 1).contiguous()
        audio_d, buf_b = audio.to(dev), bufs.to(dev)
        buf_s = [bufs[s].to(dev) for s in range(S)]
        em_b, sh_b = ctx.sola(audio_d, buf_b, block, xfade, search, delay)
        solo = [ctx.sola(audio_d[s], buf_s[s], block, xfade, search, delay) for s in range(S)]
        torch.cuda.synchronize()
        assert em_b.shape == (S, block) and sh_b.shape == (S,) and sh_b.dtype == torch.int32
        for s in range(S):
            assert torch.equal(em_b[s], solo[s][0]), (step, s)
            assert torch.equal(buf_b[s], buf_s[s]), (step, s)
            assert int(sh_b[s]) == int(solo[s][1]), (step, s)
            em_o, buf_o, sh_o = RT.sola_step(audio[s], bufs[s], block, xfade, search, delay)
            assert int(sh_b[s]) == sh_o, (step, s, int(sh_b[s]), sh_o)
            assert (em_b[s].cpu() - em_o).abs().max() < 2e-6
            assert (buf_b[s].cpu() - buf_o).abs().max() < 1e-7
        if step == 0:
            assert sh_b.tolist() == [100, 157, 311]
        bufs = buf_b.cpu()
    assert not torch.equal(bufs[0], bufs[1]) and not torch.equal(bufs[1], bufs[2])
    assert not torch.equal(em_b[0], em_b[1]) and not torch.equal(em_b[1], em_b[2])


def test_stream_push_and_phase_vocoder_batch_equal_solo(ctx, dev):
    rng = np.random.Generator(np.random.PCG64(23))
    n_in, block = 44100, 8820
    windows = torch.from_numpy(rng.standard_normal((S, n_in)).astype(np.float32)).to(dev)
    solo = [windows[s].clone() for s in range(S)]
    ptr = windows.data_ptr()
    for _ in range(3):
        blocks = torch.from_numpy(rng.standard_normal((S, block)).astype(np.float32)).to(dev)
        assert ctx.stream_push_(windows, blocks) is windows
        for s in range(S):
            ctx.stream_push_(solo[s], blocks[s].contiguous())
        torch.cuda.synchronize()
        assert windows.data_ptr() == ptr
        for s in range(S):
            assert torch.equal(windows[s], solo[s]), s
    with pytest.raises(ValueError):
        ctx.stream_push_(windows, torch.zeros(S - 1, block, device=dev))
    with pytest.raises(ValueError):
        ctx.stream_push_(windows, torch.zeros(S, n_in, device=dev))                      # block >= n_in
    n = 1764
    t = np.arange(n) / 44100
    a = np.stack([0.3 * np.sin(2 * np.pi * f * t) + 0.02 * rng.standard_normal(n) for f in TONES]).astype(np.float32)
    b = np.stack([0.3 * np.sin(2 * np.pi * f * t + 0.8 + s) + 0.02 * rng.standard_normal(n) for s, f in enumerate(TONES)]).astype(np.float32)
    a, b = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    fade_in = torch.sin(torch.pi * torch.arange(0, 1, 1 / n, device=dev)[:n] / 2) ** 2
    fade_out = 1 - fade_in
    got = ctx.phase_vocoder(a, b, fade_out, fade_in)
    torch.cuda.synchronize()
    assert got.shape == (S, n)
    for s in range(S):
        assert torch.equal(got[s], ctx.phase_vocoder(a[s], b[s], fade_out, fade_in)), s
    assert not torch.equal(got[0], got[1])


# ---- 2. row mixes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frames", [None, [33, 20, 9]], ids=["rect", "ragged"])
def test_row_mixes_against_rows_alone(dev, model, n_frames):
    import hipddsp
    Fr = 33
    inp = {k: v.to(dev) for k, v in synthetic.make_inputs(31, S, Fr).items()}
    ids, w = hipddsp.mix_rows(MIXES, 3, 100)
    assert ids.tolist() == [[2, 1, 1], [1, 5, 1], [7, 3, 4]]
    kw = {} if n_frames is None else {"n_frames": n_frames}
    with torch.no_grad():
        sig = model(inp["units"], inp["f0"], inp["volume"], None, spk_mix_rows=(ids.to(dev), w.to(dev)), noise=inp["noise"], **kw)[0]
        spk = torch.tensor([[2], [1], [7]], device=dev)
        plain = model(inp["units"], inp["f0"], inp["volume"], spk, noise=inp["noise"], **kw)[0]
        torch.cuda.synchronize()
        assert torch.equal(sig[0], plain[0])                 # the row {2: 1.0} is the plain speaker id 2
        assert not torch.equal(sig[1], plain[1]) and not torch.equal(sig[2], plain[2])
        for b, mix in enumerate(MIXES):
            n = Fr if n_frames is None else n_frames[b]
            one = lambda t: t[b:b + 1, :n].contiguous()
            how = {"spk_mix_dict": mix} if len(mix) > 1 else {}
            alone = model(one(inp["units"]), one(inp["f0"]), one(inp["volume"]), torch.tensor([[2]], device=dev),
                          noise=inp["noise"][b:b + 1, :n * 512].contiguous(), **how)[0]
            d = rms(sig[b, :n * 512] - alone[0])
            print(f"row {b} ({n} frames): rms vs the row alone {d:.3e} (signal rms {rms(alone):.3e})")
            assert rms(alone) > 1e-3
            assert d < 1e-4, (b, d)
            if n < Fr:
                assert float(sig[b, n * 512:].abs().max()) == 0.0


def test_row_mix_bad_id_is_reported_not_indexed(dev, model):
    """An id outside [1, n_spk] in a device table: the device error word, ValueError from the next poll."""
    import hipddsp
    inp = {k: v.to(dev) for k, v in synthetic.make_inputs(32, S, 9).items()}
    ids, w = hipddsp.mix_rows(MIXES, 3, 100)
    ids[1, 1] = 101
    with torch.no_grad():
        model(inp["units"], inp["f0"], inp["volume"], None, spk_mix_rows=(ids.to(dev), w.to(dev)), noise=inp["noise"])
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        hipddsp.context_for(dev).poll_error()


# ---- 3. speaker and pitch changes without a new capture ----------------------------------------------------------------------
def test_set_speaker_and_pitch_without_recapture(dev, model):
    a, b = _bank(model, 44100, dev), _bank(model, 44100, dev)
    assert a.frames == 87 and a.graph_builds == 1 and a.graph is not None
    graph = a.graph
    rng = np.random.Generator(np.random.PCG64(91))
    for k in range(BLOCKS):
        if k == 3:
            a.set_speaker(1, spk_mix_dict={1: 0.3, 5: 0.7})
            a.set_pitch(1, 3.0)
        blocks = _blocks(k, a.block, 44100, rng, silent=()).to(dev)
        units, f0, noise = _frames_inputs(k, a.frames, dev)
        ea, eb = a.push_block(blocks, units, f0, noise=noise), b.push_block(blocks, units, f0, noise=noise)
        torch.cuda.synchronize()
        assert torch.equal(ea[0], eb[0]) and torch.equal(ea[2], eb[2]), k
        assert torch.equal(ea[1], eb[1]) == (k < 3), k
        assert float(ea.abs().max()) > 0
    assert a.graph_builds == 1 and a.graph is graph
    assert a.spk_ids[1].tolist() == [1, 5, 1, 1] and abs(float(a.pitch[1]) - 2 ** 0.25) < 1e-6


# ---- 4. the bank against solo renderers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [44100, 48000])
def test_bank_against_solo_renderers(dev, model, sr):
    """Split in two: the signal before the splice is compared in RMS, the splice itself bit for bit on the bank's own signal (a
    SOLA arg-max may move between near-equal lags when the signal differs in the sixth digit; no block is skipped here)."""
    import realtime
    bank = _bank(model, sr, dev)
    pitches = (0.0, 0.0, 2.0)
    solo, seen, splicers = [], [], []
    for s, mix in enumerate(MIXES):
        how = {"spk_mix_dict": mix} if len(mix) > 1 else {"spk_id": 2}
        r = realtime.StreamRenderer(model, sr, BLOCK_TIME, XFADE_TIME, dev, buffer_num=BUFFER_NUM, threshold_db=THR, use_graph=False,
                                    pitch_adjust=pitches[s], **how)
        push, got = r.splicer.push, []
        r.splicer.push = lambda audio, push=push, got=got: (got.append(audio.clone()), push(audio))[1]
        solo.append(r)
        seen.append(got)
        splicers.append(realtime.Splicer(sr, BLOCK_TIME, XFADE_TIME, dev))
        bank.set_speaker(s, spk_mix_dict=mix) if len(mix) > 1 else bank.set_speaker(s, spk_id=2)
        bank.set_pitch(s, pitches[s])
    assert (bank.n_in, bank.frames, bank.block) == (solo[0].n_in, solo[0].frames, solo[0].block)
    rng = np.random.Generator(np.random.PCG64(91))
    loudest = 0.0
    for k in range(BLOCKS):
        blocks = _blocks(k, bank.block, sr, rng).to(dev)
        units, f0, noise = _frames_inputs(k, bank.frames, dev)
        em = bank.push_block(blocks, units, f0, noise=noise)
        torch.cuda.synchronize()
        assert em.shape == (S, bank.block) and bank.last_shift.shape == (S,)
        for s in range(S):
            solo[s].push_block(blocks[s], units=units[s:s + 1], f0=f0[s:s + 1], noise=noise[s:s + 1])
            want = seen[s][-1]
            assert bank.last_signal[s].shape == want.shape
            d = rms(bank.last_signal[s] - want)
            print(f"{sr} block {k} row {s}: signal rms vs the solo renderer {d:.3e} (signal rms {rms(want):.3e})")
            assert d < 1e-4, (k, s, d)
            e = splicers[s].push(bank.last_signal[s].contiguous())
            assert torch.equal(em[s], e), (k, s)
            assert int(bank.last_shift[s]) == int(splicers[s].last_shift), (k, s)
            loudest = max(loudest, rms(want))
        assert float(bank.last_signal[1].abs().max()) > 0 or k >= 3
    assert loudest > 1e-3 and bank.graph_builds == 1


# ---- 5. push_audio against its composition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_push_audio_equals_composition(dev, model, crepe, encoder, use_graph):
    sr = 44100
    bank = _bank(model, sr, dev, use_graph=use_graph, units_encoder=encoder, f0_extractor="crepe", crepe_ckpt=crepe, f0_dither=False)
    plain = _bank(model, sr, dev, use_graph=use_graph)
    for b in (bank, plain):
        for s, mix in enumerate(MIXES):
            b.set_speaker(s, spk_mix_dict=mix)
    windows = torch.zeros(S, bank.n_in, device=dev)
    rng = np.random.Generator(np.random.PCG64(91))
    for k in range(BLOCKS):
        blocks = _blocks(k, bank.block, sr, rng).to(dev)
        noise = synthetic.make_inputs(6000 + k, S, bank.frames)["noise"].to(dev)
        windows = torch.cat([windows[:, bank.block:], blocks], dim=1)
        f0 = bank.f0_extractor.extract(windows, uv_interp=True, silence_front=bank.silence_front, dither=False)[:, :, None]
        units = encoder.encode(windows, sr, bank.hop_size)
        em = bank.push_audio(blocks, noise=noise)
        torch.cuda.synchronize()
        assert torch.equal(bank.windows, windows), k
        assert bank.last_f0.shape == (S, bank.frames, 1) and bank.last_units.shape == (S, bank.frames, 256)
        assert bank.last_volume.shape == (S, bank.frames)
        assert torch.equal(bank.last_f0, f0), (k, float((bank.last_f0 - f0).abs().max()))
        assert torch.equal(bank.last_units, units), (k, float((bank.last_units - units).abs().max()))
        shift = bank.last_shift.clone()
        em_p = plain.push_block(blocks, units, f0, noise=noise)
        torch.cuda.synchronize()
        assert torch.equal(em, em_p), (k, float((em - em_p).abs().max()))
        assert torch.equal(shift, plain.last_shift), k
        assert float(em[0].abs().max()) > 0 or k == 0
    assert not torch.equal(em[0], em[2]) and not torch.equal(bank.last_volume[0], bank.last_volume[2])
    assert bank.graph_builds == (1 if use_graph else 0) and (bank.bank_graph is not None) == use_graph


# ---- 6. isolation -------------------------------------------------------------------------------------------------------
def test_reset_isolates_a_slot(dev, model):
    """`reset(1)` after block 2: slot 1 goes on as the slot of a bank that was fed zeros there for blocks 0-2; slots 0 and 2
    do not notice."""
    a, fresh, never = (_bank(model, 44100, dev) for _ in range(3))
    rng = np.random.Generator(np.random.PCG64(91))
    for k in range(BLOCKS):
        blocks = _blocks(k, a.block, 44100, rng, silent=()).to(dev)
        units, f0, noise = _frames_inputs(k, a.frames, dev)
        if k == 3:
            a.reset(1)
        quiet = blocks.clone()
        if k < 3:
            quiet[1] = 0
        ea = a.push_block(blocks, units, f0, noise=noise)
        ef = fresh.push_block(quiet, units, f0, noise=noise)
        en = never.push_block(blocks, units, f0, noise=noise)
        torch.cuda.synchronize()
        assert torch.equal(ea[0], en[0]) and torch.equal(ea[2], en[2]), k
        if k < 3:
            assert float(ef[1].abs().max()) == 0.0                 # an idle slot: zeros in, zeros out through the gate
        else:
            assert torch.equal(ea[1], ef[1]), k
            assert float(ea[1].abs().max()) > 0
    assert not torch.equal(ea[1], en[1])                           # (the reset did change slot 1)
    assert a.graph_builds == 1


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def test_bank_refusals_launch_nothing(dev, model, crepe, encoder):
    import realtime
    from ddsp.vocoder import F0_Extractor
    sentinel = torch.full((64,), 7.0, device=dev)
    bank = _bank(model, 44100, dev)
    state = [t.clone() for t in (bank.windows, bank.sola_buffer, bank.spk_ids, bank.spk_w, bank.pitch)]
    units, f0, noise = _frames_inputs(0, bank.frames, dev)
    bad_calls = [
        lambda: bank.push_block(torch.zeros(S, bank.block + 1, device=dev), units, f0),
        lambda: bank.push_block(torch.zeros(S - 1, bank.block, device=dev), units, f0),
        lambda: bank.push_block(torch.zeros(bank.block, device=dev), units, f0),
        lambda: bank.push_audio(torch.zeros(S, bank.block, device=dev)),                    # no analysis configured
        lambda: bank.set_speaker(S, spk_id=1),
        lambda: bank.set_speaker(-1, spk_id=1),
        lambda: bank.set_pitch(S, 1.0),
        lambda: bank.reset(S),
        lambda: bank.set_speaker(0, spk_mix_dict={1: 0.2, 2: 0.2, 3: 0.2, 4: 0.2, 5: 0.2}),    # more than max_mix = 4 ids
        lambda: bank.set_speaker(0, spk_mix_dict={1: 0.5, 101: 0.5}),
        lambda: bank.set_speaker(0, spk_id=0),
        lambda: bank.set_speaker(0, spk_id=101),
        lambda: _bank(model, 44100, dev, max_mix=0),
        lambda: _bank(model, 44100, dev, max_mix=17),
        lambda: _bank(model, 48000, dev, units_encoder=encoder,                               # an analyser at another rate
                      f0_extractor=F0_Extractor("crepe", 44100, 512 * 48000 / 44100, crepe_ckpt=crepe, device=dev)),
        lambda: _bank(model, 48000, dev, units_encoder=encoder,                               # ... at another hop
                      f0_extractor=F0_Extractor("crepe", 48000, 512, crepe_ckpt=crepe, device=dev)),
        lambda: _bank(model, 44100, dev, units_encoder=encoder),                              # half an analysis
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {i} did not raise")
    torch.cuda.synchronize()
    assert bank.graph_builds == 1
    assert torch.equal(sentinel, torch.full((64,), 7.0, device=dev))
    for t, want in zip((bank.windows, bank.sola_buffer, bank.spk_ids, bank.spk_w, bank.pitch), state):
        assert torch.equal(t, want)
    assert bank.push_block(torch.zeros(S, bank.block, device=dev), units, f0).shape == (S, bank.block)
