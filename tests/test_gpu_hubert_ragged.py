"""Ragged HuBERT-Soft (`HubertSoft.units(wav, n_samples=)` -> ddsp_hubert_soft_units with n_samples): every row of a padded batch
against the fp64 eager network (tests/hubert_cases.eager_units, the fixture's weight fill) run on THAT ROW ALONE at its own
length on the CPU - never against a call of the library.  Gates: those of tests/test_gpu_hubert.py (relative rms 5e-6 with
fp32 products, 1e-4 in split-bf16); the fp32 eager network is within 1.3e-6 of the fp64 one at every length used here.

One batch carries the lengths: B = 8, T = 41360, frame counts 1, 2, 15, 63, 64, 64, 65, 129 - a one-key softmax, rows far
shorter than the 64-frame reach of the positional convolution, both sides of the 64-key attention tile, two sample counts
with the same frame count, two full tiles and a tail, the full row; conv0 frame counts below the 1024 GroupNorm
partitions (95 for the shortest row: most partitions are empty) and above them (8287 for the full row)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import crepe_cases as CC
import hubert_cases as HC
import synthetic
from conftest import GOLDEN
from oracle import resample as OR
from test_gpu_hubert import GATES, _rel

pytestmark = pytest.mark.gpu

T = 41360
N_SAMPLES = [400, 721, 5000, 20400, 20719, 20720, 21039, 41360]
FRAMES = [1, 2, 15, 63, 64, 64, 65, 129]


def _stages(sd, wav):
    """`HC.eager_units` with its intermediates: (conv stack output (B, Fr, 512), hidden state before the first transformer
    layer (B, Fr, 768)); the same ops in the same order as the head of `eager_units`."""
    p = lambda k: sd[k]  # noqa: E731
    x = F.pad(wav.unsqueeze(1), (40, 40))
    x = F.conv1d(x, p("feature_extractor.conv0.weight"), stride=5)
    x = F.gelu(F.group_norm(x, 512, p("feature_extractor.norm0.weight"), p("feature_extractor.norm0.bias"), 1e-5))
    for i in range(1, 7):
        x = F.gelu(F.conv1d(x, p(f"feature_extractor.conv{i}.weight"), stride=2))
    conv = x.transpose(1, 2)
    x = F.layer_norm(conv, (512,), p("feature_projection.norm.weight"), p("feature_projection.norm.bias"), 1e-5)
    x = F.linear(x, p("feature_projection.projection.weight"), p("feature_projection.projection.bias"))
    v, g = p("positional_embedding.conv.weight_v"), p("positional_embedding.conv.weight_g")
    w = v * (g / v.norm(dim=(0, 1), keepdim=True))
    pos = F.conv1d(x.transpose(1, 2), w, p("positional_embedding.conv.bias"), padding=64, groups=16)[..., :-1]
    return conv, F.layer_norm(x + F.gelu(pos).transpose(1, 2), (768,), p("norm.weight"), p("norm.bias"), 1e-5)


@pytest.fixture(scope="module")
def model(dev):
    from ddsp.hubert import HubertSoft
    m = HubertSoft()
    m.load_state_dict(HC.fill({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def sd64(model):
    return {k: v.detach().cpu().double() for k, v in model.state_dict().items()}


@pytest.fixture(scope="module")
def wav():
    return torch.from_numpy((0.1 * np.random.default_rng(41).standard_normal((8, T))).astype(np.float32))


@pytest.fixture(scope="module")
def oracle(sd64, wav):
    """Per row of the batch, alone at its own length, in fp64 on the CPU: (units, conv stack output, pre-transformer state)."""
    rows = []
    with torch.no_grad():
        for b, n in enumerate(N_SAMPLES):
            x = wav[b:b + 1, :n].double()
            conv, pre = _stages(sd64, x)
            rows.append((HC.eager_units(sd64, x)[0], conv[0], pre[0]))
    return rows


@pytest.fixture(params=["fp32", "split"])
def mode(request, ctx):
    import hipddsp
    prev = ctx.math
    ctx.set_math(hipddsp.MATH_FP32 if request.param == "fp32" else hipddsp.MATH_SPLIT_BF16)
    yield request.param
    ctx.set_math(prev)


def _poisoned(wav, n_samples, dev, value=float("nan")):
    """(B, 1, T) on the device with everything past a row's own samples overwritten."""
    x = wav.clone()
    for b, n in enumerate(n_samples):
        x[b, n:] = value
    return x[:, None].to(dev)


def _check_rows(got, wants, gate, what):
    """Row b of `got` (B, Fr, C) against wants[b] (n_b, C) over its own frames; exact zeros after them; all finite."""
    got = got.cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: the output holds non-finite values"
    for b, want in enumerate(wants):
        n = want.shape[0]
        err = _rel(got[b, :n], want)
        print(f"{what} row {b} ({n} frames): relative rms {err:.3e} (gate {gate:.0e})")
        assert err <= gate, f"{what} row {b} ({n} frames): relative rms {err:.3e} (gate {gate:.0e})"
        assert torch.equal(got[b, n:], torch.zeros_like(got[b, n:])), f"{what} row {b}: the tail is not exactly 0"


def test_frame_counts_of_the_batch():
    import hipddsp
    assert [hipddsp.hubert_frames(n) for n in N_SAMPLES] == FRAMES and hipddsp.hubert_frames(T) == 129
    t0 = [(n + 80 - 10) // 5 + 1 for n in N_SAMPLES]
    assert min(t0) < 1024 < max(t0)


def test_units_of_every_row_as_if_encoded_alone(model, wav, oracle, mode, dev):
    got = model.units(_poisoned(wav, N_SAMPLES, dev), n_samples=N_SAMPLES)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (8, 129, 256)
    _check_rows(got, [o[0] for o in oracle], GATES[mode], f"units {mode}")
    # the oracle's own stages end in the oracle
    assert all(o[0].shape[0] == f and o[1].shape == (f, 512) and o[2].shape == (f, 768) for o, f in zip(oracle, FRAMES))


@pytest.mark.parametrize("padding", [float("inf"), 1e30, 0.0])
def test_padding_may_hold_anything(model, wav, dev, padding):
    want = model.units(_poisoned(wav, N_SAMPLES, dev), n_samples=N_SAMPLES)
    got = model.units(_poisoned(wav, N_SAMPLES, dev, padding), n_samples=torch.tensor(N_SAMPLES))
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_a_row_does_not_move_with_its_neighbours(model, wav, oracle, mode, dev):
    """Rows 2 (15 frames) and 4 (64 frames) of the batch again, in a batch of another B, T and other neighbours."""
    T2 = 23001
    other = torch.from_numpy((0.1 * np.random.default_rng(43).standard_normal((3, T2))).astype(np.float32))
    other[0, :N_SAMPLES[4]] = wav[4, :N_SAMPLES[4]]
    other[2, :N_SAMPLES[2]] = wav[2, :N_SAMPLES[2]]
    counts = [N_SAMPLES[4], T2, N_SAMPLES[2]]
    got = model.units(_poisoned(other, counts, dev), n_samples=counts).cpu()
    first = model.units(_poisoned(wav, N_SAMPLES, dev), n_samples=N_SAMPLES).cpu()
    assert tuple(got.shape) == (3, 71, 256) and bool(torch.isfinite(got).all())
    for here, there in ((0, 4), (2, 2)):
        n = FRAMES[there]
        for name, t in (("second batch", got[here]), ("first batch", first[there])):
            err = _rel(t[:n], oracle[there][0])
            print(f"row of {n} frames in the {name} {mode}: relative rms {err:.3e}")
            assert err <= GATES[mode], f"row of {n} frames in the {name}: relative rms {err:.3e}"
        assert not got[here, n:].any()


@pytest.mark.parametrize("layer,idx", [(-1, 1), (0, 2)])
def test_intermediates_of_every_row(model, wav, oracle, mode, dev, layer, idx):
    """layer -1 isolates conv0's selection and the GroupNorm statistics, layer 0 the positional convolution's edge."""
    got = model.encode(_poisoned(wav, N_SAMPLES, dev), layer=layer, n_samples=N_SAMPLES)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (8, 129, 512 if layer == -1 else 768)
    _check_rows(got, [o[idx] for o in oracle], GATES[mode], f"layer {layer} {mode}")


# (B, heads): the three query tiles of attention_launch at L = 129 - 32, 64 and 16 queries per workgroup
@pytest.mark.parametrize("B,H", [(5, 12), (10, 12), (5, 2)])
@pytest.mark.parametrize("math", ["fp32", "split"])
def test_softmax_attention_ragged_against_fp64(ctx, dev, B, H, math):
    import hipddsp
    L = 129
    keys = ([1, 63, 64, 65, 129] * 2)[:B]
    g = torch.Generator().manual_seed(B * 100 + H)
    q, k, v = (torch.randn(B * L, H * 64, generator=g) * s for s in (1.0, 1.0, 0.5))
    bad = torch.zeros(B, L, 1, dtype=torch.bool)
    for b, n in enumerate(keys):
        bad[b, n:] = True
    poison = lambda t: t.reshape(B, L, -1).masked_fill(bad, float("nan")).reshape(B * L, -1).to(dev)  # noqa: E731
    out = torch.full((B * L, H * 64), 7.0, device=dev)
    ret = ctx.softmax_attention(poison(q), poison(k), poison(v), B, L, H, n_keys_dev=ctx.ragged_counts(keys), out=out,
                                math=hipddsp.MATH_FP32 if math == "fp32" else hipddsp.MATH_SPLIT_BF16)
    torch.cuda.synchronize()
    assert ret.data_ptr() == out.data_ptr()
    out = out.cpu().reshape(B, L, H * 64)
    for b, n in enumerate(keys):
        sh = lambda t: t.double().reshape(B, L, H, 64)[b, :n].transpose(0, 1)  # noqa: E731
        want = (torch.softmax(sh(q) @ sh(k).transpose(-1, -2) / 8.0, dim=-1) @ sh(v)).transpose(0, 1).reshape(n, H * 64)
        err = _rel(out[b, :n], want)
        assert err <= 1e-6, f"B={B} H={H} keys={n} {math}: relative rms {err:.3e}"
        assert bool((out[b, n:] == 7.0).all()), f"keys={n}: rows past the count were written"


def test_rectangular_call_is_untouched(model, wav, sd64, oracle, mode, dev):
    """`units(wav)` and `units(wav, n_samples=[T] * B)` against the fp64 network on the full rows; `units(wav)` bit for bit
    the same before and after ragged calls."""
    with torch.no_grad():
        want = [HC.eager_units(sd64, wav[0:1].double())[0], oracle[7][0]]
    ragged = model.units(wav[[0, 7], None].to(dev), n_samples=[T, T])
    rect = model.units(wav[[0, 7], None].to(dev))
    again = model.units(wav[[0, 7], None].to(dev))
    torch.cuda.synchronize()
    assert torch.equal(rect, again)
    for b in range(2):
        for name, t in (("rectangular", rect), ("n_samples=[T]*B", ragged)):
            err = _rel(t[b], want[b])
            assert err <= GATES[mode], f"{name} row {b} {mode}: relative rms {err:.3e}"


_FRESH_PROCESS = """
import sys
sys.path[:0] = {paths!r}
import numpy as np, torch
import hubert_cases as HC
from ddsp.hubert import HubertSoft
dev = torch.device("cuda:0")
m = HubertSoft()
m.load_state_dict(HC.fill({{k: tuple(v.shape) for k, v in m.state_dict().items()}}), strict=True)
m = m.to(dev).eval()
wav = torch.from_numpy((0.1 * np.random.default_rng(41).standard_normal((3, 1, 21039))).astype(np.float32)).to(dev)
first = m.units(wav)                                  # before any ragged call in this process
ragged = m.units(wav, n_samples=[400, 21039, 20719])
a, b = m.units(wav), m.units(wav)
torch.cuda.synchronize()
assert bool(ragged[1].any()) and not bool(ragged[0, 1:].any())
print("BITS", bool(torch.equal(a, b)), bool(torch.equal(a, first)))
"""


def test_rectangular_bits_before_and_after_ragged_calls(lib_path):
    """`units(wav)` twice after a ragged call: bit for bit each other, and the rectangular call made before any ragged call
    in the process - a fresh process, so that no earlier test of a run decides what 'before' means."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [os.path.join(root, "ddsp-svc-official_amd"), os.path.join(root, "tests"), root]
    r = subprocess.run([sys.executable, "-c", _FRESH_PROCESS.format(paths=paths)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert "BITS True True" in r.stdout, r.stdout[-500:]


def test_a_device_tensor_of_counts_is_refused(model, wav, dev):
    with pytest.raises(ValueError):
        model.units(wav[:, None].to(dev), n_samples=torch.tensor(N_SAMPLES, device=dev))
    with pytest.raises(ValueError):
        model.units(wav[:, None].to(dev), n_samples=N_SAMPLES[:-1] + [T + 1])
    with pytest.raises(ValueError):
        model.units(wav[:, None].to(dev), n_samples=[319] + N_SAMPLES[1:])


# ---- Units_Encoder.encode(..., n_samples=) ---------------------------------------------------------------------------
SR, HOP = 44100, 512


def _encoder(model, tmp_path, dev):
    from ddsp.vocoder import Units_Encoder
    path = str(tmp_path / "hubert-soft.pt")
    torch.save({"module." + k: v.detach().cpu() for k, v in model.state_dict().items()}, path)
    return Units_Encoder("hubertsoft", path, device=dev)


def _solo_encode64(sd64, audio, sample_rate, hop_size):
    """`Units_Encoder.encode` of ONE row alone restated on the host in fp64: the resampler's formulas
    (oracle/resample.py, as tests/test_gpu_resample.py uses them), the eager network, nearest-frame indexing with the
    fp32 product and round-half-even of the reference's `torch.round(ratio * arange)`."""
    with torch.no_grad():
        x16 = OR.resample(audio[None].double(), sample_rate, 16000, 128, dtype=torch.float64) if sample_rate != 16000 \
            else audio[None].double()
        units = HC.eager_units(sd64, x16)[0]
    n = int(audio.shape[-1] // hop_size) + 1
    ratio = torch.tensor((hop_size / sample_rate) / (320 / 16000), dtype=torch.float32)
    idx = torch.clamp(torch.round(ratio * torch.arange(n, dtype=torch.float32)).long(), max=units.shape[0] - 1)
    return units[idx]


def test_units_encoder_ragged_against_the_solo_chain(model, sd64, tmp_path, dev, ctx):
    import hipddsp
    fix = np.load(os.path.join(GOLDEN, "ref_hubert_soft.npz"))
    counts = [2000, 22050, 57000]
    audio = torch.from_numpy((0.1 * np.random.default_rng(47).standard_normal((3, 57000))).astype(np.float32))
    padded = audio.clone()
    for b, n in enumerate(counts):
        padded[b, n:] = float("nan")
    prev = ctx.math
    ctx.set_math(hipddsp.MATH_FP32)
    try:
        enc = _encoder(model, tmp_path, dev)
        got = enc.encode(padded.to(dev), SR, HOP, n_samples=counts)
        torch.cuda.synchronize()
    finally:
        ctx.set_math(prev)
    assert tuple(got.shape) == (3, 57000 // HOP + 1, 256)
    wants = [_solo_encode64(sd64, audio[b, :n], SR, HOP) for b, n in enumerate(counts)]
    assert [w.shape[0] for w in wants] == [n // HOP + 1 for n in counts]
    _check_rows(got, wants, GATES["fp32"] + float(fix["err32_short"]), "Units_Encoder.encode")


# ---- infer_offline.convert_batched(..., units_batch_samples=) --------------------------------------------------------
# five slices of unequal length, each well under a second: from 0; after a gap; overlapping the previous one; two more
SLICES = [(0, 9000), (12000, 30000), (29000, 40000), (47000, 75000), (76000, 88000)]


def _file_audio():
    rng = np.random.default_rng(53)
    t = np.arange(2 * SR) / SR
    f = 110.0 * np.exp(np.log(4.0) * t / t[-1])
    ph = 2 * np.pi * np.cumsum(f) / SR
    return (0.3 * np.sin(ph) + 0.15 * np.sin(2 * ph + 0.3) + 0.02 * rng.standard_normal(len(t))).astype(np.float32)


def test_convert_batched_with_ragged_units(model, sd64, tmp_path, dev):
    """The whole file with the units encoded in ragged groups against the same stitch (`render`) fed, per slice, the units
    of the fp64 host chain; `units_batch_samples=None` is `convert`."""
    import hipddsp
    import infer_offline
    from ddsp.crepe import Crepe
    from ddsp.vocoder import DotDict, F0_Extractor
    crepe = Crepe("tiny")
    crepe.load_state_dict(CC.fill("tiny"))
    extractor = F0_Extractor("crepe", SR, HOP, 65.0, 800.0, crepe_ckpt=crepe, device=dev)
    encoder = _encoder(model, tmp_path, dev)
    synth, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    spk = torch.full((1, 1), 2, dtype=torch.int64, device=dev)
    audio = _file_audio()
    run = lambda f, *a, **kw: (torch.manual_seed(17), f(synth, args, audio, SR, SLICES, encoder, extractor, spk, *a,  # noqa: E731
                                                        noise_seed=5, **kw))[1]
    plain, _ = run(infer_offline.convert)
    same, _ = run(infer_offline.convert_batched, None, units_batch_samples=None)
    assert np.array_equal(plain, same)
    budget = 60000
    lengths = [b // HOP * HOP - a // HOP * HOP for a, b in SLICES]
    groups = infer_offline.group_segments(lengths, budget)
    assert 1 < len(groups) < len(SLICES) and max(len(g) for g in groups) >= 2       # real groups, more than one
    got, sr_o = run(infer_offline.convert_batched, None, units_batch_samples=budget)
    # ragged from the raw audio to the waveform: against the ragged synthesis fed per-slice units (a ragged group draws its
    # noise from the group's seed, so the per-slice stitch is not its reference)
    both, _ = run(infer_offline.convert_batched, 4096, units_batch_samples=budget)
    synth_only, _ = run(infer_offline.convert_batched, 4096)
    x = torch.from_numpy(audio)
    torch.manual_seed(17)
    f0 = extractor.extract(x.to(dev), uv_interp=True)[None, :, None]
    volume = hipddsp.context_for(dev).volume_extract(x[None].to(dev), HOP)
    segments = [(a // HOP, _solo_encode64(sd64, x[a // HOP * HOP:b // HOP * HOP], SR, HOP)[None].float().to(dev))
                for a, b in SLICES]
    want, sr_w = infer_offline.render(synth, args, segments, f0, volume, spk, noise_seed=5)
    assert sr_o == sr_w == SR and got.dtype == np.float64 and got.shape == want.shape == plain.shape == both.shape
    assert float(np.abs(want).max()) > 1e-3
    for name, y, ref in (("ragged units", got, want), ("per-slice loop", plain, want),
                         ("ragged units and ragged synthesis", both, synth_only)):
        err = float(np.sqrt(np.mean((y - ref) ** 2)))
        print(f"{name}: rms error of the file {err:.3e} (signal rms {float(np.sqrt(np.mean(want ** 2))):.3e})")
        assert err <= 1e-4, f"{name}: rms error {err:.3e}"


# ---- graph capture ------------------------------------------------------------------------------------------------------
def test_ragged_units_replay_bit_identically_under_graph_capture(model, wav, dev):
    """Fixed counts, checked and uploaded before the capture (`HubertSoft.counts`): nothing is uploaded or read back inside."""
    import hipddsp
    x = _poisoned(wav, N_SAMPLES, dev)
    gctx = hipddsp.Context(dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s), hipddsp.use_context(gctx):
        counts = model.counts(N_SAMPLES, 8, T, dev)
        eager = model.units(x, n_samples=counts)
        eager = model.units(x, n_samples=counts)   # warm-up: scratch arena at size
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = model.units(x, n_samples=counts)
    gctx.freeze()
    torch.cuda.current_stream(dev).wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager), f"max |diff| {float((out - eager).abs().max()):.3e}"
    assert torch.equal(eager.cpu(), model.units(x, n_samples=N_SAMPLES).cpu())
