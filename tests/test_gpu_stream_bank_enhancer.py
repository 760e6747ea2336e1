"""The enhancer stage of `realtime.StreamBank`: the three keyed kernels against their solo forms, `Enhancer.enhance_keyed` per
row against `Enhancer.enhance`, the bank against solo `StreamRenderer`s while rows change key, and the captured stage against
the eager one.

Bank geometry: that of tests/test_gpu_stream_bank.py (S = 3, 'config5': 0.2 s blocks, 87 frames at 44.1 kHz, 6 blocks).
Enhancer: the narrow synthetic checkpoint of tests/test_gpu_enhancer_ragged.py (hop 32, n_fft 128, 44.1 kHz).  The callers' f0
rows are near-constant tracks, so that every block's key is known: 220 Hz (key 0; key 3 after a shift of two octaves), 1000 Hz
(key 5) and 800 Hz (key 1)."""
import json

import numpy as np
import pytest
import torch

import glue_cases as GC
import synthetic
from conftest import rms

pytestmark = pytest.mark.gpu
S, BLOCKS = 3, 6
BLOCK_TIME, XFADE_TIME, BUFFER_NUM = 0.2, 0.04, 4          # 'config5'
THR = -45.0
RI = torch.tensor([0.0, 0.3, 0.7, 0.1, 0.9, 0.5, 0.2, 0.8, 0.4])


def _rate(k, sr_e=44100):
    return 100 * int(np.round(sr_e * 2 ** (k / 12) / 100))


def _host_key(f0_row, cut, request, max_key):
    import hipddsp
    if request >= 0:
        return min(request, max_key)
    return hipddsp.key_from_thresholds(float(np.max(f0_row[cut:])), hipddsp.key_thresholds(max_key))


@pytest.fixture(scope="module")
def enh(dev, lib_path, tmp_path_factory):
    from enhancer import Enhancer
    tmp = tmp_path_factory.mktemp("nsf")
    with open(tmp / "config.json", "w") as fh:
        json.dump(dict(GC.NSF_CONFIG), fh)
    torch.save({"generator": GC.nsf_state_dict()}, tmp / "model")
    return Enhancer("nsf-hifigan", str(tmp / "model"), device=dev)


@pytest.fixture(scope="module")
def model(dev, lib_path):
    return synthetic.build_model("CombSub", seed=43, device=dev)[0]


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [0, 3])
def test_enhancer_keys_against_the_host_rule(ctx, dev, cut):
    import hipddsp
    Fr = 18
    for edge in (759.99, 760.0, 760.01):
        f0 = np.zeros((6, Fr), dtype=np.float32)
        f0[1] = 220.0
        f0[2, :3], f0[2, 3:] = 800.0, 300.0            # the peak lies inside the cut of 3 frames
        f0[3] = 500.0
        f0[3, 11] = edge
        f0[4] = 5000.0                                 # clamped to max_key
        f0[5] = 1000.0                                 # a fixed key 2 is asked for this row
        request = [-1, -1, -1, -1, -1, 2]
        for max_key in (12, 4, 1):
            thr = torch.from_numpy(hipddsp.key_thresholds(max_key)).to(dev)
            got = ctx.enhancer_keys(torch.from_numpy(f0).to(dev), cut, max_key, ctx.ragged_counts(request), thr)
            assert got.dtype == torch.int32 and got.shape == (6,)
            want = [_host_key(f0[s], cut, request[s], max_key) for s in range(6)]
            assert got.tolist() == want, (edge, cut, max_key, got.tolist(), want)
            if max_key == 12:
                assert want == [0, 0, 1 if cut == 0 else 0, 0 if edge <= 760.0 else 1, 12, 2]


@pytest.mark.parametrize("direction", ["to_working_rate", "back"])
def test_resample_keyed_rows_equal_solo_bit_for_bit(ctx, dev, direction):
    B, T = 5, 3000
    n, keys = [3000, 2999, 1, 1500, 700], [0, 1, 5, 12, 5]
    pairs = [(44100, _rate(k)) if direction == "to_working_rate" else (_rate(k), 44100) for k in range(13)]
    length = ctx.lib.ddsp_resample_length
    rng = np.random.Generator(np.random.PCG64(5))
    x = torch.full((B, T), float("nan"))
    for b in range(B):
        x[b, :n[b]] = torch.from_numpy(rng.standard_normal(n[b]).astype(np.float32))
    x = x.to(dev)
    plan = ctx.resample_plan(pairs, 128)
    assert plan.length(T) == max(T if a == b else length(T, a, b) for a, b in pairs)
    want = []
    for b in range(B):
        a, c = pairs[keys[b]]
        row = x[b:b + 1, :n[b]].contiguous()
        want.append(row[0] if a == c else ctx.resample(row, a, c, 128)[0])         # equal rates: the row itself
        assert want[-1].numel() == (n[b] if a == c else length(n[b], a, c))
    n_dev, k_dev = ctx.ragged_counts(n), ctx.ragged_counts(keys)

    def check(tag):
        got = ctx.resample_keyed(plan, x, n_dev, k_dev)
        torch.cuda.synchronize()
        assert got.shape == (B, plan.length(T))
        for b in range(B):
            m = want[b].numel()
            assert torch.equal(got[b, :m], want[b]), (tag, b)
            assert torch.equal(got[b, m:], torch.zeros_like(got[b, m:])), (tag, b, "the tail of a row must be exactly 0")
        return got

    first = check("first")
    assert float(first[0].abs().max()) > 0 and not torch.equal(first[2, :8], first[4, :8])
    # a key outside the set is clamped into it before it indexes anything
    wild = ctx.resample_keyed(plan, x, n_dev, ctx.ragged_counts([-7, 1, 5, 99, 5]))
    assert torch.equal(wild, first)
    for i in range(8):                               # eight other pairs go through the solo cache of 8 tables
        ctx.resample(x[:1, :64].nan_to_num(0.0).contiguous(), 16000 + 100 * i, 22050, 16)
    assert torch.equal(check("after the solo cache turned over"), first)


def test_retime_f0_keyed_rows_equal_ragged(ctx, dev):
    rng = np.random.Generator(np.random.PCG64(32))
    ns, nd, keys = [87, 27, 1, 40], [173, 120, 5, 700], [0, 3, 12, 5]
    scales = [44100 / _rate(k) for k in range(13)]
    f0 = np.full((4, max(ns)), np.nan, dtype=np.float32)
    for b, m in enumerate(ns):
        f0[b, :m] = rng.uniform(60, 1900, m).astype(np.float32)
    f0 = torch.from_numpy(f0).to(dev)
    ns_d, nd_d = ctx.ragged_counts(ns), ctx.ragged_counts(nd)
    div = torch.tensor(scales, dtype=torch.float64).to(dev)
    scale = torch.tensor(scales, dtype=torch.float32).to(dev)
    got = ctx.retime_f0(f0, 512 / 44100, None, None, 32 / 44100, max(nd), n_src_dev=ns_d, n_dst_dev=nd_d,
                        keyed=(ctx.ragged_counts(keys), div, scale))
    assert got.shape == (4, max(nd))
    for b, k in enumerate(keys):
        want = ctx.retime_f0(f0, 512 / 44100, scales[k], scales[k], 32 / 44100, max(nd), n_src_dev=ns_d, n_dst_dev=nd_d)
        assert torch.equal(got[b], want[b]), b
        assert not got[b, nd[b]:].any() and float(got[b, :nd[b]].min()) > 0
    assert not torch.equal(got[0, :5], got[1, :5])


# ---- 2. enhance_keyed against enhance -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("silence_front", [0, 0.03], ids=["whole", "front_cut"])
def test_enhance_keyed_rows_against_solo_enhance(dev, enh, silence_front):
    T, hop = 8192, 512
    Fr = T // hop
    tones = (220.0, 800.0, 1000.0, 0.0)
    audio = GC.nsf_audio(T, seed=810).repeat(4, 1).to(dev)
    f0 = torch.stack([torch.full((Fr, 1), f) + (0.5 * torch.sin(torch.arange(Fr) / 3.0))[:, None] * (f > 0) for f in tones]).to(dev)
    if silence_front:
        assert enh._front_cut(silence_front, 44100, hop)[0] == 2
    plan = enh.keyed_plan(T, Fr, 44100, hop, silence_front, 12)
    got, sr_e, n_out, key = enh.enhance_keyed(audio, 44100, f0, hop, adaptive_key="auto", silence_front=silence_front, rand_ini=RI,
                                              plan=plan)
    torch.cuda.synchronize()
    assert sr_e == 44100 and key.tolist() == [0, 1, 5, 0] and n_out.dtype == torch.int32 and key.dtype == torch.int32
    assert got.shape == (4, max(plan.n_out))
    for s in range(4):
        want, sr_w = enh.enhance(audio[s:s + 1], 44100, f0[s:s + 1], hop, adaptive_key=int(key[s]), silence_front=silence_front,
                                 rand_ini=RI)
        m = want.shape[-1]
        assert sr_w == sr_e and int(n_out[s]) == m, (s, int(n_out[s]), m)
        d = rms(got[s, :m] - want[0])
        print(f"silence_front {silence_front} row {s} (key {int(key[s])}, {m} samples): rms vs enhance {d:.3e} (signal rms {rms(want):.3e})")
        assert rms(want) > 1e-3
        assert d <= 1e-4, (s, d)
        assert torch.equal(got[s, m:], torch.zeros_like(got[s, m:])), (s, "everything past n_out must be exactly 0")
    assert len(set(n_out.tolist())) > 1
    # requests as a device tensor: a fixed key for row 0, 'auto' for the others; one number for all rows
    req = torch.tensor([4, -1, -1, -1], dtype=torch.int32).to(dev)
    assert enh.enhance_keyed(audio, 44100, f0, hop, adaptive_key=req, silence_front=silence_front, rand_ini=RI, plan=plan)[3].tolist() == [4, 1, 5, 0]
    assert enh.enhance_keyed(audio, 44100, f0, hop, adaptive_key=2, silence_front=silence_front, rand_ini=RI, plan=plan)[3].tolist() == [2] * 4


# ---- 3. the bank --------------------------------------------------------------------------------------------------------------
TRACKS = (220.0, 1000.0, 800.0)


def _inputs(k, bank, dev):
    """Block k: blocks (S, block) of tones, the callers' units, f0 (near-constant tracks, so that the keys are known) and noise."""
    rng = np.random.Generator(np.random.PCG64(300 + k))
    t = (np.arange(bank.block) + k * bank.block) / bank.samplerate
    blocks = np.stack([0.2 * np.sin(2 * np.pi * f * t) + 0.01 * rng.standard_normal(bank.block) for f in (147.0, 220.0, 330.0)])
    z = synthetic.make_inputs(8000 + k, S, bank.frames)
    wob = 1.0 + 0.004 * torch.sin(torch.arange(bank.frames) / 4.0 + k)
    f0 = torch.stack([f * wob for f in TRACKS])[:, :, None]
    return torch.from_numpy(blocks.astype(np.float32)).to(dev), z["units"].to(dev), f0.to(dev), z["noise"].to(dev)


def _bank(model, sr, dev, **kw):
    import realtime
    return realtime.StreamBank(model, S, sr, BLOCK_TIME, XFADE_TIME, dev, buffer_num=BUFFER_NUM, threshold_db=THR, **kw)


def _expected_keys(k):
    return [0 if k < 3 else 3, 5 if k < 4 else 0, 1]


@pytest.mark.parametrize("sr", [44100, 48000])
def test_bank_with_enhancer_against_solo_renderers(dev, model, enh, sr):
    """As test_bank_against_solo_renderers: the tail before the splice in RMS against the solo renderer (which is given the
    block's key as a number), the splice bit for bit on the bank's own tail.  Row 0 goes up two octaves at block 3 (key 0 -> 3),
    row 1 is fixed to key 0 at block 4 (from 'auto' = 5)."""
    import realtime
    bank = _bank(model, sr, dev, enhancer=enh)
    n_tail = bank.block + bank.xfade + bank.search + bank.delay
    solo, seen, splicers = [], [], []
    for s in range(S):
        r = realtime.StreamRenderer(model, sr, BLOCK_TIME, XFADE_TIME, dev, buffer_num=BUFFER_NUM, threshold_db=THR, use_graph=False,
                                    spk_id=1, enhancer=enh, enhancer_adaptive_key=0)
        push, got = r.splicer.push, []
        r.splicer.push = lambda audio, push=push, got=got: (got.append(audio.clone()), push(audio))[1]
        solo.append(r)
        seen.append(got)
        splicers.append(realtime.Splicer(sr, BLOCK_TIME, XFADE_TIME, dev))
    loudest = 0.0
    for k in range(BLOCKS):
        if k == 3:
            bank.set_pitch(0, 24.0)
            solo[0].pitch_adjust = 24.0
        if k == 4:
            bank.set_enhancer_key(1, 0)
        blocks, units, f0, noise = _inputs(k, bank, dev)
        em = bank.push_block(blocks, units, f0, noise=noise, rand_ini=RI)
        torch.cuda.synchronize()
        assert em.shape == (S, bank.block) and bank.last_signal.shape == (S, n_tail)
        assert bank.last_key.tolist() == _expected_keys(k), (k, bank.last_key.tolist())
        for s in range(S):
            solo[s].enhancer_adaptive_key = _expected_keys(k)[s]
            solo[s].push_block(blocks[s], units=units[s:s + 1], f0=f0[s:s + 1], noise=noise[s:s + 1], rand_ini=RI)
            want = seen[s][-1][-n_tail:]
            d = rms(bank.last_signal[s] - want)
            print(f"{sr} block {k} row {s} key {_expected_keys(k)[s]}: tail rms vs the solo renderer {d:.3e} (signal rms {rms(want):.3e})")
            assert d <= 1e-4, (k, s, d)
            e = splicers[s].push(bank.last_signal[s].contiguous())
            assert torch.equal(em[s], e), (k, s)
            assert int(bank.last_shift[s]) == int(splicers[s].last_shift), (k, s)
            loudest = max(loudest, rms(want))
        assert not torch.equal(em[0], em[1]) and not torch.equal(em[1], em[2]) and not torch.equal(em[0], em[2])
    assert loudest > 1e-3 and bank.graph_builds == 1 and bank.enhancer_graph is not None


def test_captured_stage_equals_eager_and_plain_bank_is_unchanged(ctx, dev, model, enh):
    sr = 48000
    eager, graph = _bank(model, sr, dev, enhancer=enh, use_graph=False), _bank(model, sr, dev, enhancer=enh, use_graph=True)
    plain = _bank(model, sr, dev)
    assert plain.enhancer is None and plain.enhancer_graph is None and plain.last_key is None
    assert eager.graph_builds == 0 and graph.graph_builds == 1
    windows, buf = torch.zeros(S, plain.n_in, device=dev), torch.zeros(S, plain.xfade, device=dev)
    for k in range(BLOCKS):
        if k == 3:
            for b in (eager, graph, plain):
                b.set_pitch(0, 24.0)
        if k == 4:
            eager.set_enhancer_key(1, 0)
            graph.set_enhancer_key(1, 0)
        blocks, units, f0, noise = _inputs(k, eager, dev)
        ee = eager.push_block(blocks, units, f0, noise=noise, rand_ini=RI)
        eg = graph.push_block(blocks, units, f0, noise=noise, rand_ini=RI).clone()
        torch.cuda.synchronize()
        assert torch.equal(ee, eg), (k, float((ee - eg).abs().max()))
        assert torch.equal(eager.last_key, graph.last_key) and graph.last_key.tolist() == _expected_keys(k), k
        assert float(ee.abs().max()) > 0
        # the bank without an enhancer: the composition of the parent's push_block, bit for bit
        ep = plain.push_block(blocks, units, f0, noise=noise)
        ctx.stream_push_(windows, blocks)
        volume = ctx.volume_extract(windows, plain.hop_size)
        with torch.no_grad():
            sig = model(units, f0 * plain.pitch[:, None, None], volume, None, spk_mix_rows=(plain.spk_ids, plain.spk_w), noise=noise)[0]
        ctx.volume_gate_(sig, volume, THR, 512)
        want, _ = ctx.sola(ctx.resample(sig, 44100, sr, 128), buf, plain.block, plain.xfade, plain.search, plain.delay)
        torch.cuda.synchronize()
        assert torch.equal(ep, want), (k, float((ep - want).abs().max()))
    assert graph.graph_builds == 1 and eager.graph_builds == 0 and plain.graph_builds == 1
    with pytest.raises(ValueError):
        graph.set_enhancer_key(0, 13)
    with pytest.raises(ValueError):
        graph.set_enhancer_key(0, "automatic")
    with pytest.raises(ValueError):
        plain.set_enhancer_key(0, 1)
