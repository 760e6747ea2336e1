"""The end of an offline conversion on the device: `ddsp_stitch` against the reference's host loop (tests/golden/stitch_ref.npz)
and the numpy statement of its rule (`test_stitch_host.fold`), `ddsp_volume_gate_rows` against the per-slice gate of
`render`, and `render_device` / `convert_device` / `main.run` against `render` / `convert_batched`.

Agreement of the stitch: bit for bit everywhere, inside cross-fades too (the kernel forms the blend from rounded fp64
operations in numpy's order).  Every comparison prints the largest deviation inside the fades before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

import glue_cases as GC
import hubert_cases as HC
import stitch_cases as SC
import synthetic
from conftest import GOLDEN
from test_stitch_host import fold, load_case

pytestmark = pytest.mark.gpu
SR, HOP = synthetic.SR, synthetic.HOP
NAN = float("nan")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "stitch_ref.npz"))


def _assert_stitched(got, want, p, fade, what):
    """got == want bit for bit; the deviation inside the fade regions is printed first."""
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    inside = np.zeros(len(want), dtype=bool)
    for at, f in zip(p, fade):
        inside[at:at + f] = True
    dev_in = float(np.abs(got - want)[inside].max()) if inside.any() else 0.0
    print(f"{what}: {len(want)} samples, {int(inside.sum())} inside fades, largest deviation there {dev_in:.3e}")
    assert np.array_equal(got[~inside], want[~inside]), (what, "outside the fades")
    assert np.array_equal(got, want), (what, "inside the fades", dev_in)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_stitch_every_piece_in_its_own_tensor(dev, lib_path, ref, name):
    import infer_offline
    sr, sr_o, starts, pieces, want = load_case(ref, name)
    plan = infer_offline.stitch_plan(starts, [len(x) for x in pieces], SC.BLOCK, sr, sr_o)
    got = infer_offline.stitch([torch.from_numpy(x.copy()).to(dev) for x in pieces], plan, device=dev)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (plan[2],)
    _assert_stitched(got.cpu().numpy(), want, plan[0], plan[1], name)


@pytest.mark.parametrize("name", [n for n in SC.CASES if n != "empty"])
def test_stitch_rows_of_two_padded_groups(dev, lib_path, ref, name):
    """The pieces as rows of two padded group tensors, rows in shuffled order, T_max = 43 (no multiple of 4: odd rows start at
    odd offsets) and every piece one sample into its row: the table's addresses and the scalar path.  The padding is NaN: a
    read outside a piece would show in the result."""
    import infer_offline
    sr, sr_o, starts, pieces, want = load_case(ref, name)
    order = np.random.Generator(np.random.PCG64(77)).permutation(len(pieces))
    members = [[i for k, i in enumerate(order) if k % 2 == g] for g in (0, 1)]
    views = [None] * len(pieces)
    for rows in members:
        group = torch.full((max(len(rows), 1), 43), NAN, device=dev)
        for r, i in enumerate(rows):
            group[r, 1:1 + len(pieces[i])] = torch.from_numpy(pieces[i].copy()).to(dev)
            views[i] = group[r:r + 1, 1:1 + len(pieces[i])]
    plan = infer_offline.stitch_plan(starts, [len(x) for x in pieces], SC.BLOCK, sr, sr_o)
    _assert_stitched(infer_offline.stitch(views, plan).cpu().numpy(), want, plan[0], plan[1], name + " (group rows)")


def test_stitch_larger_file_against_the_numpy_statement(dev, lib_path):
    """42 pieces of 1 to 3000 samples in about 8e4 output samples (some eighty workgroups of 1024: the binary search and
    tiles that hold several pieces or a part of one), gaps, abutting pieces, fades of 1 to a whole piece and a piece over
    two earlier ones; the pieces lie at arbitrary offsets of one NaN-filled buffer, so aligned and unaligned loads both run."""
    import infer_offline
    rng = np.random.Generator(np.random.PCG64(4242))
    lengths = [int(n) for n in rng.integers(1, 3001, size=42)]
    lengths[0], lengths[5], lengths[6], lengths[7], lengths[20], lengths[30] = 3000, 1, 2, 3, 3000, 1
    starts, cur, prev = [], 0, 0
    for i, n in enumerate(lengths):
        kind = i % 4
        most = min(n, cur - prev)                       # a fade may reach back to the previous piece's start, not further
        f = 0 if kind < 2 or most < 1 else (1 if i % 8 == 3 else int(rng.integers(1, most + 1)))
        at = cur + (int(rng.integers(1, 60)) if kind == 0 else 0) - f
        starts.append(at)
        prev, cur = at, at + n
    # a piece over two earlier ones: the last three are (p, len) = (cur, 30), (cur + 25, 10), (cur + 28, 20)
    for at, n in ((cur, 30), (cur + 25, 10), (cur + 28, 20)):
        starts.append(at)
        lengths.append(n)
    pieces = [(0.5 * rng.standard_normal(n)).astype(np.float32) for n in lengths]
    p, fade, total = infer_offline.stitch_plan(starts, lengths, 1, SR, SR)
    assert total <= 100000 and len(pieces) == 45 and 1 in fade and max(fade) >= 100 and min(lengths) == 1
    assert fade[-2:] == [5, 7] and any(f == n for f, n in zip(fade, lengths))
    buf = torch.full((sum(lengths) + 4 * len(lengths),), NAN, device=dev)
    views, off = [], 0
    for i, x in enumerate(pieces):
        off += i % 4                                     # the piece's address modulo 16 bytes walks through 0, 4, 8, 12
        buf[off:off + len(x)] = torch.from_numpy(x).to(dev)
        views.append(buf[off:off + len(x)])
        off += len(x)
    got = infer_offline.stitch(views, (p, fade, total))
    _assert_stitched(got.cpu().numpy(), fold(p, fade, pieces, total), p, fade, "larger file")


def test_stitch_of_nothing_is_empty(dev, lib_path):
    import infer_offline
    got = infer_offline.stitch([], infer_offline.stitch_plan([], [], 4, SR, SR), device=dev)
    assert got.shape == (0,) and got.dtype == torch.float64 and got.is_cuda


# ---- the gate of a ragged group ----------------------------------------------------------------------------------------

def _gate_case(dev):
    """volume (30,) over the threshold at frames 0, 3-4 and 29 (the dilation reaches both edges of the file); rows from
    frames 0, 5 and 21 with 4, 9 and 9 frames, and a fourth from frame 4 with 5 whose last frame (8) ramps towards the file's
    frame 9; T_max = 10 * 512; the signal is noise with the padding of every row at 7.25."""
    vol = torch.full((30,), 1e-4)
    vol[[0, 3, 4, 29]] = 0.1
    starts, counts = [0, 5, 21, 4], [4, 9, 9, 5]
    rng = np.random.Generator(np.random.PCG64(606))
    sig = torch.from_numpy(rng.standard_normal((4, 10 * 512)).astype(np.float32))
    for b, n in enumerate(counts):
        sig[b, n * 512:] = 7.25
    return vol.to(dev), starts, counts, sig.to(dev)


def test_volume_gate_rows_equals_the_per_slice_gate(ctx, dev, lib_path):
    import infer_offline
    vol, starts, counts, sig = _gate_case(dev)
    want = sig.clone()
    for b, (s, n) in enumerate(zip(starts, counts)):     # the existing path, as `render` applies it
        out = want[b:b + 1, :n * 512]
        out *= infer_offline.volume_mask(vol[None], -60, 512)[:, s * 512:(s + n) * 512]
    got = ctx.volume_gate_rows_(sig.clone(), vol, ctx.ragged_counts(starts), ctx.ragged_counts(counts), -60, 512)
    assert torch.equal(got, want)
    for b, n in enumerate(counts):
        assert bool((got[b, n * 512:] == 7.25).all()), b
    # the gate does something: row 1 is open at its start and shut at its end, row 3 ramps down inside its own last frame
    assert torch.equal(got[1, :512], sig[1, :512]) and not got[1, 5 * 512:9 * 512].any()
    assert torch.equal(got[3, :4 * 512], sig[3, :4 * 512]) and float(got[3, 5 * 512 - 1].abs()) < float(sig[3, 5 * 512 - 1].abs()) * 0.01
    torch.cuda.synchronize()
    ctx.poll_error()


def test_volume_gate_rows_reports_a_row_outside_the_file(ctx, dev, lib_path):
    vol, starts, counts, sig = _gate_case(dev)
    torch.cuda.synchronize()
    ctx.poll_error()
    before = sig.clone()
    got = ctx.volume_gate_rows_(sig, vol, ctx.ragged_counts([0, 5, 22, 4]), ctx.ragged_counts(counts), -60, 512)   # 22 + 9 > 30
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="ddsp_volume_gate_rows"):
        ctx.poll_error()
    ctx.poll_error()                                      # reported once
    assert torch.equal(got[2], before[2])                 # the row was left alone


# ---- render_device / convert_device / main ---------------------------------------------------------------------------------

def _fixed_enhancer(tmp_path, dev):
    """The small NSF-HiFiGAN of tests/test_gpu_enhancer_ragged.py from a checkpoint on disk, its random initial phases pinned."""
    from enhancer import Enhancer
    with open(tmp_path / "config.json", "w") as fh:
        json.dump(dict(GC.NSF_CONFIG), fh)
    torch.save({"generator": GC.nsf_state_dict()}, tmp_path / "model")
    ri = torch.tensor([0.0, 0.3, 0.7, 0.1, 0.9, 0.5, 0.2, 0.8, 0.4])

    class Fixed(Enhancer):
        def enhance(self, *a, **k):
            return super().enhance(*a, rand_ini=ri, **k)

        def enhance_batch(self, *a, **k):
            return super().enhance_batch(*a, rand_ini=ri, **k)

    return Fixed("nsf-hifigan", str(tmp_path / "model"), device=dev)


def _fades_of(segments, lengths, sr_o):
    import infer_offline
    return infer_offline.stitch_plan([s for s, _ in segments], lengths, HOP, SR, sr_o)


def _four_slices(dev):
    """-> (the positional arguments of `render`, segments, their frame counts, keywords with the injected noise)."""
    from ddsp.vocoder import DotDict
    starts, lens = [0, 8, 13, 19], [9, 3, 5, 7]
    model, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    whole = synthetic.make_inputs(913, 1, 40, with_noise=False)
    whole["volume"][0, 20:32] = 0.0
    rng = np.random.Generator(np.random.PCG64(914))
    segments = [(s, torch.from_numpy(rng.standard_normal((1, n, 256), dtype=np.float32)).to(dev)) for s, n in zip(starts, lens)]
    noise = [torch.from_numpy(rng.random(n * HOP, dtype=np.float32)).to(dev) for n in lens]
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    common = (model, args, segments, whole["f0"].to(dev), whole["volume"].to(dev), whole["spk_id"].to(dev))
    return common, segments, lens, dict(noise=noise, batch_frames=16)


@pytest.mark.parametrize("with_enhancer", [False, True])
def test_render_device_equals_render(dev, lib_path, tmp_path, with_enhancer):
    """Four slices of 9, 3, 5 and 7 frames (the second overlaps the first by a frame: a cross-fade; gaps behind the second and
    third), injected noise, volume shut over frames 20-31 so the gate bites inside the last slice; `batch_frames` and
    `enhancer_batch_samples` the same on both sides."""
    import infer_offline
    common, segments, lens, kw = _four_slices(dev)
    if with_enhancer:
        kw.update(enhancer=_fixed_enhancer(tmp_path, dev), enhancer_batch_samples=8000)
    want, sr_w = infer_offline.render(*common, **kw)
    got, sr_o = infer_offline.render_device(*common, **kw)
    assert sr_o == sr_w and got.is_cuda and got.dtype == torch.float64 and float(np.abs(want).max()) > 1e-3
    if not with_enhancer:
        p, fade, total = _fades_of(segments, [n * HOP for n in lens], sr_o)
        assert fade == [0, HOP, 0, 0] and total == 26 * HOP == len(want)
        assert not want[24 * HOP:].any() and want[19 * HOP:20 * HOP].any()      # the gate shut the end of the last slice
    else:
        # the fades lie where the enhancer's piece lengths put them, which the result does not tell: every sample is held to
        # equality, as if none were inside a fade
        p, fade = [], []
    _assert_stitched(got.cpu().numpy(), want, p, fade, f"render_device (enhancer {with_enhancer})")


def test_render_device_passes_the_speaker_mix_to_the_model(dev, lib_path):
    """`spk_mix_dict` goes through the one render body untouched: the four slices with a mix of two speakers, against `render`
    with the same dictionary; the mix is not the call's `spk_id` alone."""
    import infer_offline
    common, segments, lens, kw = _four_slices(dev)
    mix = {1: 0.5, 2: 0.5}
    want, sr_w = infer_offline.render(*common, spk_mix_dict=mix, **kw)
    got, sr_o = infer_offline.render_device(*common, spk_mix_dict=mix, **kw)
    plain, _ = infer_offline.render_device(*common, **kw)
    assert sr_o == sr_w == SR and float(np.abs(want).max()) > 1e-3 and not torch.equal(got, plain)
    p, fade, _ = _fades_of(segments, [n * HOP for n in lens], sr_o)
    _assert_stitched(got.cpu().numpy(), want, p, fade, "render_device (speaker mix)")


def _voiced(n, f_lo, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    ph = 2 * np.pi * np.cumsum(f_lo * np.exp(np.log(2.0) * t / t[-1])) / SR
    return 0.3 * np.sin(ph) + 0.15 * np.sin(2 * ph + 0.3) + 0.02 * rng.standard_normal(n)


@pytest.fixture(scope="module")
def encoder(dev, lib_path, tmp_path_factory):
    from ddsp.hubert import HubertSoft
    from ddsp.vocoder import Units_Encoder
    path = str(tmp_path_factory.mktemp("hubert") / "hubert-soft.pt")
    torch.save(HC.fill({k: tuple(v.shape) for k, v in HubertSoft().state_dict().items()}), path)
    return Units_Encoder("hubertsoft", path, device=dev)


def _speech_and_silence():
    """3 s in the manner of tests/test_gpu_slicer.py: 2 s of a harmonic tone, then 1 s of noise floor that is quietest from 2.3 to
    2.5 s - with main.py's defaults the slicer tags the trailing silence there, so `split` gives a voiced and a silence range."""
    rng = np.random.default_rng(41)
    t = np.arange(2 * SR) / SR
    voiced = 0.3 * np.sin(2 * np.pi * 190.7 * t) + 0.1 * np.sin(2 * np.pi * 381.4 * t + 0.3) + 1e-3 * rng.standard_normal(len(t))
    floor = 1e-4 * rng.standard_normal(SR)
    floor[int(0.3 * SR):int(0.5 * SR)] *= 0.1
    return np.concatenate([voiced, floor]).astype(np.float32)


@pytest.mark.parametrize("slices", [[(0, 40000), (45000, 90000), (88000, 132300)], None])
def test_convert_device_equals_convert_batched(dev, lib_path, encoder, slices):
    """The same inputs through `convert_batched` and `convert_device`: given slices (from 0; behind a gap; overlapping the one
    before) on 3 s of audio, and `slices=None` (the device slicer) on 3 s that end in a silence."""
    import infer_offline
    from ddsp.vocoder import DotDict, F0_Extractor
    extractor = F0_Extractor("ac", SR, HOP, 65.0, 800.0, device=dev)
    model, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    spk = torch.full((1, 1), 2, dtype=torch.int64, device=dev)
    audio = _speech_and_silence() if slices is None else _voiced(3 * SR, 110.0, 31).astype(np.float32)
    common = (model, args, audio, SR, slices, encoder, extractor, spk, 96)
    kw = dict(key=3, noise_seed=5, units_batch_samples=60000)
    want, sr_w = infer_offline.convert_batched(*common, **kw)
    got, sr_o = infer_offline.convert_device(*common, **kw)
    assert sr_o == sr_w == SR and float(np.abs(want).max()) > 1e-3
    if slices is None:
        found = infer_offline.split(torch.from_numpy(audio).to(dev), SR, HOP)
        assert len(found) == 2, found
        p, fade = [], []
    else:
        frames = [(a // HOP, b // HOP - a // HOP + 1) for a, b in slices]      # (start frame, frames of units)
        p, fade, total = infer_offline.stitch_plan([s for s, _ in frames], [n * HOP for _, n in frames], HOP, SR, SR)
        assert fade == [0, 0, 5 * HOP] and total == len(want)
    _assert_stitched(got.cpu().numpy(), want, p, fade, f"convert_device (slices {'given' if slices else 'None'})")


@pytest.mark.parametrize("units_batch_samples", [None, 60000])
def test_convert_device_at_a_fractional_hop(dev, lib_path, encoder, units_batch_samples):
    """1 s at 48 kHz into a 44.1 kHz / 512 model: the hop is 557.28 samples, legal for ONE file.  The second slice starts at
    sample 23962, no multiple of 4, so the gather of the encoder's rows takes its unaligned loads; both slices share a group."""
    import infer_offline
    from ddsp.vocoder import DotDict, F0_Extractor
    sr_in, slices = 48000, [(0, 20000), (24000, 48000)]
    hop = HOP * sr_in / SR
    pieces = infer_offline.piece_table([slices], hop)
    assert not float(hop).is_integer() and [row[1:] for row in pieces] == [(0, 35, 0, 19504), (43, 44, 23962, 23963)]
    extractor = F0_Extractor("ac", sr_in, hop, 65.0, 800.0, device=dev)
    model, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    spk = torch.full((1, 1), 2, dtype=torch.int64, device=dev)
    common = (model, args, _voiced(sr_in, 110.0, 31).astype(np.float32), sr_in, slices, encoder, extractor, spk, 96)
    kw = dict(key=3, noise_seed=5, units_batch_samples=units_batch_samples)
    want, sr_w = infer_offline.convert_batched(*common, **kw)
    got, sr_o = infer_offline.convert_device(*common, **kw)
    assert sr_o == sr_w == SR and float(np.abs(want).max()) > 1e-3
    p, fade, total = infer_offline.stitch_plan([row[1] for row in pieces], [row[2] * HOP for row in pieces], HOP, SR, SR)
    assert total == len(want) == 87 * HOP
    _assert_stitched(got.cpu().numpy(), want, p, fade, f"convert_device (hop {hop:.2f}, units_batch_samples {units_batch_samples})")
    if units_batch_samples is None:                       # the gather at unaligned starts, against the encoder on torch slices
        x = torch.from_numpy(common[2]).to(dev)
        segments, _, _ = infer_offline._analyse(args, common[2], sr_in, slices, encoder, extractor, 3, None)
        for (start, units), (_, start_frame, n, at, n_samples) in zip(segments, pieces):
            assert start == start_frame and units.shape[1] == n
            assert torch.equal(units, encoder.encode(x[None, at:at + n_samples], sr_in, hop)), start


def test_a_given_slice_that_reaches_past_the_file_is_cut_at_its_end(dev, lib_path, encoder):
    """A detector's last slice rounded past T (3 s, 132300 samples; the slice ends at 135300): the one-file calls cut it at the
    file's end as the Python slice of main.py:41-46 does - 44748 samples from 87552, 88 frames of units, the file's last frame
    included - and do not refuse it.  The units against the encoder on the torch slice, bit for bit; then the whole chain."""
    import infer_offline
    from ddsp.vocoder import DotDict, F0_Extractor
    extractor = F0_Extractor("ac", SR, HOP, 65.0, 800.0, device=dev)
    model, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    spk = torch.full((1, 1), 2, dtype=torch.int64, device=dev)
    audio = _voiced(3 * SR, 110.0, 31).astype(np.float32)
    slices = [(0, 40000), (88000, len(audio) + 3000)]
    x = torch.from_numpy(audio).to(dev)
    segments, f0, _ = infer_offline._analyse(args, audio, SR, slices, encoder, extractor, 0, None)
    assert [(s, u.shape[1]) for s, u in segments] == [(0, 79), (171, 88)] and f0.shape[1] == 259
    assert torch.equal(segments[1][1], encoder.encode(x[None, 171 * HOP:], SR, HOP))
    common = (model, args, audio, SR, slices, encoder, extractor, spk, 96)
    kw = dict(key=3, noise_seed=5, units_batch_samples=60000)
    want, _ = infer_offline.convert_batched(*common, **kw)
    got, _ = infer_offline.convert_device(*common, **kw)
    assert len(want) == 259 * HOP and float(np.abs(want).max()) > 1e-3
    _assert_stitched(got.cpu().numpy(), want, [], [], "convert_device (a slice past the end)")


def test_main_run_writes_the_converted_file(dev, lib_path, encoder, tmp_path):
    """`main.run` on a model directory made here (config.yaml and a seeded CombSub checkpoint), `-pe ac -e false`, the units
    encoder injected: the file holds the 16-bit samples of the returned waveform, which is `convert_device`'s for the loaded
    model under the same generator state (the model draws its noise seed from torch's generator)."""
    import yaml
    from scipy.io import wavfile

    import infer_offline
    import main
    from ddsp.vocoder import F0_Extractor, load_model
    model, _ = synthetic.build_model("CombSub", seed=8, device="cpu")
    cfg = {"data": {"sampling_rate": SR, "block_size": HOP, "encoder": "hubertsoft", "encoder_ckpt": "unused", "encoder_sample_rate": 16000,
                    "encoder_hop_size": 320, "encoder_out_channels": 256},
           "model": dict(synthetic.MODEL_CFG["CombSub"], c=False), "enhancer": {"type": "nsf-hifigan", "ckpt": "unused"}}
    with open(tmp_path / "config.yaml", "w") as fh:
        yaml.safe_dump(cfg, fh)
    torch.save({"global_step": 0, "model": model.state_dict()}, tmp_path / "model_0.pt")
    audio = _voiced(2 * SR, 130.0, 9).astype(np.float32)
    wavfile.write(tmp_path / "in.wav", SR, audio)
    cmd = main.parse_args(["-m", str(tmp_path / "model_0.pt"), "-i", str(tmp_path / "in.wav"), "-o", str(tmp_path / "out.wav"),
                           "-pe", "ac", "-e", "false", "-k", "2", "-id", "3"])
    torch.manual_seed(41)
    result, sr_o = main.run(cmd, units_encoder=encoder, device=dev)
    rate, written = wavfile.read(tmp_path / "out.wav")
    assert rate == sr_o == SR and written.dtype == np.int16 and result.dtype == torch.float64 and result.is_cuda
    assert np.array_equal(written, main.pcm16(result.cpu().numpy())) and int(np.abs(written).max()) > 30
    assert len(written) == (len(audio) // HOP + 1) * HOP
    torch.manual_seed(41)                                 # as in `run`: the model's construction draws from the generator too
    loaded, args = load_model(str(tmp_path / "model_0.pt"), device=dev)
    want, _ = infer_offline.convert_device(loaded, args, torch.from_numpy(audio).to(dev), SR, None, encoder,
                                           F0_Extractor("ac", SR, HOP, 50.0, 1100.0, device=dev),
                                           torch.full((1, 1), 3, dtype=torch.int64, device=dev), batch_frames=4096, key=2.0)
    assert torch.equal(result, want)
