"""Offline conversion of several files at once on the device: `ddsp_pieces_gather` against torch slicing, the gate of rows of
several files (`ddsp_volume_gate_files`) against `volume_gate_rows_` on every row's file alone, `render_many_device` against
`render_device` per file, `analyse_many` against `_analyse` per file, the `noise_seed` rule, files without slices.

Bounds are quoted, not made here: a ragged row against the row alone is held to rms < 1e-4 (`GATE` of tests/test_gpu_ragged.py;
no test there holds a ragged row to its solo render bit for bit, so a group of rows of several files is held to that gate too),
units of another grouping to the relative rms of tests/test_gpu_hubert_ragged.py (`GATES["split"]` of tests/test_gpu_hubert.py).
Where the many-file call makes the very launches of the per-file call (one slice per group) the results are held bit for bit."""
import numpy as np
import pytest
import torch

import hubert_cases as HC
import synthetic
from conftest import rms
from test_gpu_hubert import GATES, _rel
from test_gpu_ragged import GATE

pytestmark = pytest.mark.gpu
SR, HOP = synthetic.SR, synthetic.HOP
NAN = float("nan")


def _i32(ctx, rows):
    return torch.tensor(rows, dtype=torch.int32).to(ctx.device)


# ---- the gather kernel alone -------------------------------------------------------------------------------------------------

N_SAMPLES, N_FRAMES, KEYS = [700, 2051, 5], [11, 33, 1], [0, 3, -12]
# (file, start_frame, n_frames, start_sample, n_samples): an odd start (unaligned loads); one sample, ending on its file's last
# sample and frame; a second piece of that file, aligned (row 1 of audio starts at float 2051, and 2051 + 129 = 4 * 545); a
# whole tiny file; a piece ending on its file's last sample and frame, aligned too
PIECES = [(0, 0, 4, 1, 255), (1, 30, 3, 2050, 1), (1, 2, 17, 129, 1100), (2, 0, 1, 0, 5), (0, 5, 6, 300, 400)]


def _gather_case(dev):
    rng = np.random.Generator(np.random.PCG64(515))
    audio = torch.full((3, max(N_SAMPLES)), NAN)
    f0, volume = torch.full((3, max(N_FRAMES)), NAN), torch.full((3, max(N_FRAMES)), NAN)
    for k, (n, fr) in enumerate(zip(N_SAMPLES, N_FRAMES)):
        audio[k, :n] = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
        f0[k, :fr] = torch.from_numpy(rng.uniform(80.0, 700.0, fr).astype(np.float32))
        volume[k, :fr] = torch.from_numpy(rng.random(fr).astype(np.float32))
    factor = torch.tensor([2 ** (float(key) / 12) for key in KEYS], dtype=torch.float32)
    return audio.to(dev), f0.to(dev), volume.to(dev), factor.to(dev)


@pytest.mark.parametrize("S_max,N_max", [(1100, 17), (1101, 19), (1103, 20)])
def test_pieces_gather_equals_torch_slicing(ctx, dev, lib_path, S_max, N_max):
    """Row widths that are and are not multiples of 4 (odd rows of wav then start at unaligned addresses: the scalar stores)."""
    audio, f0, volume, factor = _gather_case(dev)
    ns_dev, nf_dev = _i32(ctx, N_SAMPLES), _i32(ctx, N_FRAMES)
    wav, f0_rows, vol_rows = ctx.pieces_gather(_i32(ctx, PIECES), ns_dev, nf_dev, audio=audio, S_max=S_max, f0=f0, volume=volume,
                                               key_factor=factor, N_max=N_max)
    assert wav.shape == (5, S_max) and f0_rows.shape == vol_rows.shape == (5, N_max)
    for r, (k, sf, nf, ss, ns) in enumerate(PIECES):
        assert torch.equal(wav[r, :ns], audio[k, ss:ss + ns]) and not wav[r, ns:].any(), r
        want = f0[k, sf:sf + nf] * torch.tensor(2 ** (KEYS[k] / 12)).to(dev)      # one rounded fp32 product per element
        assert torch.equal(f0_rows[r, :nf], want) and not f0_rows[r, nf:].any(), r
        assert torch.equal(vol_rows[r, :nf], volume[k, sf:sf + nf]) and not vol_rows[r, nf:].any(), r
    assert torch.equal(f0_rows[0, :4], f0[0, :4])                                 # key 0 leaves the bits
    assert not torch.equal(f0_rows[1, :3], f0[1, 30:33])
    # each half alone
    only_wav = ctx.pieces_gather(_i32(ctx, PIECES), ns_dev, nf_dev, audio=audio, S_max=S_max)
    only_frames = ctx.pieces_gather(_i32(ctx, PIECES), ns_dev, nf_dev, f0=f0, volume=volume, key_factor=factor, N_max=N_max)
    assert torch.equal(only_wav[0], wav) and only_wav[1] is None and only_frames[0] is None
    assert torch.equal(only_frames[1], f0_rows) and torch.equal(only_frames[2], vol_rows)
    torch.cuda.synchronize()
    ctx.poll_error()


@pytest.mark.parametrize("bad", [(0, 5, 6, 300, 401), (0, 5, 7, 300, 400), (3, 0, 1, 0, 1), (1, 2, 17, 129, 1101), (1, -1, 2, 0, 4)])
def test_pieces_gather_reports_a_piece_outside_its_file(ctx, dev, lib_path, bad):
    """One sample or one frame past the file's own end (still inside the padded batch, where NaN lies), a file index past the
    batch, more samples than the row holds, a negative frame: a row of zeros, the other rows as they should be, DDSP_ERR_ARG."""
    import hipddsp
    audio, f0, volume, factor = _gather_case(dev)
    torch.cuda.synchronize()
    ctx.poll_error()
    pieces = [PIECES[0], bad, PIECES[3]]
    wav, f0_rows, vol_rows = ctx.pieces_gather(_i32(ctx, pieces), _i32(ctx, N_SAMPLES), _i32(ctx, N_FRAMES), audio=audio, S_max=1100,
                                               f0=f0, volume=volume, key_factor=factor, N_max=17)
    torch.cuda.synchronize()
    assert ctx.lib.ddsp_ctx_poll_error(ctx.handle) == hipddsp.DDSP_ERR_ARG
    assert b"ddsp_pieces_gather" in ctx.lib.ddsp_last_error(ctx.handle)
    ctx.poll_error()                                                              # reported once
    assert not wav[1].any() and not f0_rows[1].any() and not vol_rows[1].any()
    assert torch.equal(wav[0, :255], audio[0, 1:256]) and torch.equal(wav[2, :5], audio[2, :5])
    assert torch.isfinite(wav).all() and torch.isfinite(f0_rows).all() and torch.isfinite(vol_rows).all()


# ---- the gate of rows of several files -----------------------------------------------------------------------------------

GATE_HOP = 64
GATE_FRAMES = [12, 20, 14]
# (file, start_frame, n_frames): from a file's first frame, up to its last frame (its interpolation), inside
GATE_ROWS = [(0, 0, 6), (1, 0, 9), (2, 0, 14), (1, 11, 9), (2, 9, 5), (0, 7, 5), (1, 5, 3)]


def _gate_files(dev):
    """File 0: loud at frames 3-4, its padding silent.  File 1: its first and last frame loud - file 0's padding, which lies in
    front of it in memory, is silent - and its own padding loud.  File 2, the reverse: loud at frame 6 alone, so frames 0-1 and
    11-13 are shut, while file 1's padding in front of it and its own padding behind it are loud: a dilation that went on to
    Fr_max would open its last frames."""
    vol = torch.full((3, 30), 1e-4)
    vol[0, [3, 4]] = 0.1
    vol[1, [0, 19]] = 0.1
    vol[1, 20:] = 0.1
    vol[2, 6] = 0.1
    vol[2, 14:] = 0.1
    rng = np.random.Generator(np.random.PCG64(616))
    sig = torch.from_numpy(rng.standard_normal((len(GATE_ROWS), 15 * GATE_HOP)).astype(np.float32))
    for b, (_, _, n) in enumerate(GATE_ROWS):
        sig[b, n * GATE_HOP:] = 7.25
    return vol.to(dev), sig.to(dev)


def test_gate_of_several_files_equals_the_gate_of_each_file_alone(ctx, dev, lib_path):
    vol, sig = _gate_files(dev)
    want = sig.clone()
    for b, (k, s, n) in enumerate(GATE_ROWS):
        alone = vol[k, :GATE_FRAMES[k]].clone()
        want[b:b + 1] = ctx.volume_gate_rows_(sig[b:b + 1].clone(), alone, _i32(ctx, [s]), _i32(ctx, [n]), -60, GATE_HOP)
    cols = list(zip(*GATE_ROWS))
    got = ctx.volume_gate_rows_(sig.clone(), vol, _i32(ctx, cols[1]), _i32(ctx, cols[2]), -60, GATE_HOP,
                                file_dev=_i32(ctx, cols[0]), file_frames_dev=_i32(ctx, GATE_FRAMES))
    assert torch.equal(got, want)
    for b, (_, _, n) in enumerate(GATE_ROWS):
        assert bool((got[b, n * GATE_HOP:] == 7.25).all()), b
    # the edges do what the files say: file 1 is open at both ends, file 2 shut at both
    assert torch.equal(got[1, :GATE_HOP], sig[1, :GATE_HOP]) and torch.equal(got[3, 8 * GATE_HOP:9 * GATE_HOP], sig[3, 8 * GATE_HOP:9 * GATE_HOP])
    assert not got[2, :GATE_HOP].any() and not got[2, 12 * GATE_HOP:14 * GATE_HOP].any() and not got[4, 3 * GATE_HOP:5 * GATE_HOP].any()
    assert got[2, 6 * GATE_HOP:7 * GATE_HOP].any()
    torch.cuda.synchronize()
    ctx.poll_error()


@pytest.mark.parametrize("bad", [(0, 7, 6), (3, 0, 2), (-1, 0, 2), (2, 0, 16)])
def test_gate_of_several_files_reports_a_bad_row(ctx, dev, lib_path, bad):
    """Past the file's own 12 frames though inside Fr_max; a file index outside the batch; more samples than the row has."""
    vol, sig = _gate_files(dev)
    torch.cuda.synchronize()
    ctx.poll_error()
    rows = [GATE_ROWS[0], bad, GATE_ROWS[1]]
    cols = list(zip(*rows))
    before = sig[:3].clone()
    got = ctx.volume_gate_rows_(sig[:3].clone(), vol, _i32(ctx, cols[1]), _i32(ctx, cols[2]), -60, GATE_HOP,
                                file_dev=_i32(ctx, cols[0]), file_frames_dev=_i32(ctx, GATE_FRAMES))
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="ddsp_volume_gate_files"):
        ctx.poll_error()
    ctx.poll_error()
    assert torch.equal(got[1], before[1]) and not torch.equal(got[2], before[2])      # the rows around it were gated


# ---- render_many_device against render_device, per file ----------------------------------------------------------------------

FILE_FRAMES = [12, 40, 5]
# file 0: one slice of 9 frames; file 1: 20 and 11 frames, the second a frame into the first (a cross-fade); file 2: 2 frames
SLICES = [(0, 1, 9), (1, 0, 20), (1, 19, 11), (2, 2, 2)]
SPK = [1, 3, 2]


def _analysed(dev, seed=77, frames=FILE_FRAMES, slices=SLICES, keys=KEYS):
    """What `analyse_many` returns, made of seeded inputs (no analysis): NaN in the padding of f0 and volume."""
    import hipddsp
    ctx = hipddsp.context_for(dev)
    rng = np.random.Generator(np.random.PCG64(seed))
    F = len(frames)
    f0, volume = torch.full((F, max(frames)), NAN), torch.full((F, max(frames)), NAN)
    for k, n in enumerate(frames):
        inp = synthetic.make_inputs(seed + k, 1, n, with_noise=False)
        f0[k, :n], volume[k, :n] = inp["f0"][0, :, 0], inp["volume"][0]
    volume[1, 21:34] = 0.0                                  # shut from 21 to 33: dilated, the gate is 0 over frames 25-28
    pieces = [(k, s, n, s * HOP, (n - 1) * HOP) for k, s, n in slices]
    units = [torch.from_numpy(rng.standard_normal((1, n, 256), dtype=np.float32)).to(dev) for _, _, n in slices]
    noise = [[torch.from_numpy(rng.random(n * HOP, dtype=np.float32)).to(dev) for j, _, n in slices if j == k] for k in range(F)]
    n_samples = [(n - 1) * HOP + 7 for n in frames]
    files = dict(hop_size=float(HOP), sample_rate=SR, device=torch.device(dev), pieces=pieces, units=units, n_samples=n_samples,
                 n_frames=list(frames), f0=f0.to(dev), volume=volume.to(dev), n_samples_dev=ctx.ragged_counts(n_samples),
                 n_frames_dev=ctx.ragged_counts(list(frames)),
                 key_factor=torch.tensor([2 ** (float(key) / 12) for key in keys], dtype=torch.float32).to(dev))
    return files, noise


def _per_file_renders(model, args, files, noise, spk, **kw):
    import infer_offline
    out = []
    for k in range(len(files["n_frames"])):
        segments, f0, volume = infer_offline.file_features(files, k)
        got, sr_o = infer_offline.render_device(model, args, segments, f0, volume, torch.full((1, 1), spk[k], dtype=torch.int64,
                                                                                                device=f0.device),
                                                noise=noise[k], **kw)
        out.append(got)
    return out


@pytest.mark.parametrize("name", ["CombSub", "Sins", "CombSubFast"])
def test_render_many_device_equals_render_device_per_file(dev, lib_path, name):
    import infer_offline
    from ddsp.vocoder import DotDict
    model, _ = synthetic.build_model(name, seed=8, device=dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    files, noise = _analysed(dev)
    groups = infer_offline.group_pieces(files["pieces"], 22)
    assert any(len({files["pieces"][i][0] for i in g}) > 1 for g in groups), groups       # rows of two files in one group
    for batch_frames in (22, None):
        got, spans, sr_o = infer_offline.render_many_device(model, args, files, SPK, noise=noise, batch_frames=batch_frames)
        want = _per_file_renders(model, args, files, noise, SPK, batch_frames=batch_frames)
        assert sr_o == SR and got.is_cuda and got.dtype == torch.float64 and len(spans) == 3
        covered = torch.zeros(got.numel(), dtype=torch.bool, device=got.device)
        for k, (base, total) in enumerate(spans):
            assert base % 2 == 0 and total == want[k].numel() and float(want[k].abs().max()) > 1e-3
            e = rms((got[base:base + total] - want[k]).cpu())
            print(name, "batch_frames", batch_frames, "file", k, "frames", total // HOP, "rms", e)
            if batch_frames is None:                      # a slice per group on both sides: the same launches, the same bits
                assert torch.equal(got[base:base + total], want[k]), (k, e)
            assert e < GATE, (k, e)
            covered[base:base + total] = True
        assert got.numel() == spans[-1][0] + spans[-1][1] and not got[~covered].any()      # the alignment gaps are exact zeros
        assert [t for _, t in spans] == [10 * HOP, 30 * HOP, 4 * HOP]
        assert not got[spans[1][0] + 26 * HOP:spans[1][0] + 28 * HOP].any()               # the gate shut file 1's frames 26-27
    torch.cuda.synchronize()
    infer_offline.hipddsp.context_for(dev).poll_error()


def test_speaker_mix_per_file(dev, lib_path):
    """`spk_mix_rows` tables with one row per file whose mix is a single speaker of weight 1 give what `spk_ids` gives."""
    import infer_offline
    from ddsp.vocoder import DotDict
    model, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    files, noise = _analysed(dev)
    a, spans, _ = infer_offline.render_many_device(model, args, files, SPK, noise=noise, batch_frames=22)
    mix = (torch.tensor(SPK, dtype=torch.int32).reshape(3, 1).to(dev), torch.ones(3, 1, device=dev))
    b, spans_b, _ = infer_offline.render_many_device(model, args, files, None, spk_mix_rows=mix, noise=noise, batch_frames=22)
    assert spans == spans_b and rms((a - b).cpu()) < GATE and float(a.abs().max()) > 1e-3


def test_noise_seed_repeats_and_identical_files_draw_different_noise(dev, lib_path):
    import infer_offline
    from ddsp.vocoder import DotDict
    model, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    files, _ = _analysed(dev, frames=[12, 12, 12], slices=[(0, 1, 9), (1, 1, 9), (2, 1, 9)], keys=[0, 0, 0])
    files["f0"][1:], files["volume"][1:] = files["f0"][0], files["volume"][0]
    files["units"] = [files["units"][0]] * 3
    still = [[torch.full((9 * HOP,), 0.5, device=dev)] for _ in range(3)]           # u = 0.5 is no noise: 2u - 1 = 0
    for batch_frames in (18, None):                       # files 0 and 1 in one group and file 2 in the next; a group each
        a, spans, _ = infer_offline.render_many_device(model, args, files, 2, noise_seed=5, batch_frames=batch_frames)
        b, _, _ = infer_offline.render_many_device(model, args, files, 2, noise_seed=5, batch_frames=batch_frames)
        quiet, _, _ = infer_offline.render_many_device(model, args, files, 2, noise=still, batch_frames=batch_frames)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
        parts = [(a - quiet)[base:base + total] for base, total in spans]
        harmonic = [quiet[base:base + total] for base, total in spans]
        assert rms((harmonic[0] - harmonic[1]).cpu()) < GATE and rms((harmonic[0] - harmonic[2]).cpu()) < GATE
        for i, j in ((0, 1), (0, 2), (1, 2)):
            assert rms(parts[i].cpu()) > 0 and rms((parts[i] - parts[j]).cpu()) > 0.5 * rms(parts[i].cpu()), (batch_frames, i, j)
    c, _, _ = infer_offline.render_many_device(model, args, files, 2, noise_seed=6, batch_frames=18)
    assert not torch.equal(a, c)


def test_a_file_without_slices_and_an_empty_list(dev, lib_path):
    import infer_offline
    from ddsp.vocoder import DotDict, F0_Extractor
    model, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    files, noise = _analysed(dev, slices=[(0, 1, 9), (2, 2, 2)])
    assert [len(x) for x in noise] == [1, 0, 1]
    got, spans, _ = infer_offline.render_many_device(model, args, files, SPK, noise=noise, batch_frames=22)
    assert [t for _, t in spans] == [10 * HOP, 0, 4 * HOP] and spans[1][0] == spans[2][0] == 10 * HOP
    want = _per_file_renders(model, args, files, noise, SPK, batch_frames=22)
    assert want[1].numel() == 0 and rms((got[spans[2][0]:] - want[2]).cpu()) < GATE
    none, _ = _analysed(dev, slices=[])
    out, spans, sr_o = infer_offline.render_many_device(model, args, none, SPK, batch_frames=22)
    assert out.numel() == 0 and out.dtype == torch.float64 and spans == [(0, 0)] * 3 and sr_o == SR
    extractor = F0_Extractor("ac", SR, HOP, 65.0, 800.0, device=dev)
    empty = infer_offline.analyse_many(args, [], SR, None, None, extractor, 0, None)
    out, spans, sr_o = infer_offline.render_many_device(model, args, empty, [], batch_frames=22)
    assert out.numel() == 0 and out.dtype == torch.float64 and out.is_cuda and spans == [] and sr_o == SR
    waves, sr_o = infer_offline.convert_many(model, args, [], SR, None, extractor, [])
    assert waves == [] and sr_o == SR


# ---- analyse_many against _analyse, per file -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def encoder(dev, lib_path, tmp_path_factory):
    from ddsp.hubert import HubertSoft
    from ddsp.vocoder import Units_Encoder
    path = str(tmp_path_factory.mktemp("hubert") / "hubert-soft.pt")
    torch.save(HC.fill({k: tuple(v.shape) for k, v in HubertSoft().state_dict().items()}), path)
    return Units_Encoder("hubertsoft", path, device=dev)


def _voiced(n, f_lo, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    ph = 2 * np.pi * np.cumsum(f_lo * np.exp(np.log(2.0) * t / t[-1])) / SR
    return (0.3 * np.sin(ph) + 0.15 * np.sin(2 * ph + 0.3) + 0.02 * rng.standard_normal(n)).astype(np.float32)


def _tone_then_floor():
    """2 s of a tone, then 1 s of noise floor that is quietest from 2.3 to 2.5 s (tests/test_gpu_stitch.py): two slices."""
    rng = np.random.default_rng(41)
    t = np.arange(2 * SR) / SR
    voiced = 0.3 * np.sin(2 * np.pi * 190.7 * t) + 0.1 * np.sin(2 * np.pi * 381.4 * t + 0.3) + 1e-3 * rng.standard_normal(len(t))
    floor = 1e-4 * rng.standard_normal(SR)
    floor[int(0.3 * SR):int(0.5 * SR)] *= 0.1
    return np.concatenate([voiced, floor]).astype(np.float32)


def test_analyse_many_equals_analyse_per_file_and_converts(dev, lib_path, encoder):
    """Three files of 3 s (two slices by the device slicer), 0.7 s and 1.3 s, keys 0, +3 and -12: f0, volume and the slice
    tables exact, the units - another grouping than the file's own - within the ragged units' gate.  Then the whole chain."""
    import infer_offline
    from ddsp.vocoder import DotDict, F0_Extractor
    extractor = F0_Extractor("ac", SR, HOP, 65.0, 800.0, device=dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    audios = [_tone_then_floor(), _voiced(int(0.7 * SR) + 3, 140.0, 5), _voiced(int(1.3 * SR), 110.0, 6)]
    files = infer_offline.analyse_many(args, audios, SR, None, encoder, extractor, KEYS, 60000)
    assert [row[0] for row in files["pieces"]] == [0, 0, 1, 2]
    for k, audio in enumerate(audios):
        segments, f0, volume = infer_offline._analyse(args, audio, SR, None, encoder, extractor, KEYS[k], 60000)
        got_segments, got_f0, got_volume = infer_offline.file_features(files, k)
        assert torch.equal(got_f0, f0) and torch.equal(got_volume, volume), k
        assert [(s, u.shape) for s, u in got_segments] == [(s, u.shape) for s, u in segments], k
        for (s, got), (_, want) in zip(got_segments, segments):
            err = _rel(got, want)
            print(f"file {k} slice at frame {s}: units relative rms {err:.3e}")
            assert err <= GATES["split"], (k, s, err)
        assert not files["f0"][k, files["n_frames"][k]:].any() and not files["volume"][k, files["n_frames"][k]:].any()
    given = infer_offline.analyse_many(args, audios, SR, [[(0, 40000), (45000, 90000)], [], [(512, 30000)]], encoder, extractor,
                                       3, None)
    assert [row[:3] for row in given["pieces"]] == [(0, 0, 79), (0, 87, 89), (2, 1, 58)]
    assert bool((given["key_factor"] == given["key_factor"][0]).all())
    with pytest.raises(ValueError, match="file 1"):
        infer_offline.analyse_many(args, audios, SR, [[], [(0, 40000)], []], encoder, extractor, 0, None)
    # the chain: every file as long as `convert_device` makes it, the sound of the same model within the ragged gate where
    # the noise is not drawn (CombSub's noise branch aside, the harmonic part dominates: the files are held to be finite and
    # as long; the parity of the rendering is test_render_many_device_equals_render_device_per_file's)
    model, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    waves, sr_o = infer_offline.convert_many(model, args, audios, SR, encoder, extractor, SPK, keys=KEYS, batch_frames=300,
                                             noise_seed=5, units_batch_samples=60000)
    assert sr_o == SR and len(waves) == 3
    for k, audio in enumerate(audios):
        alone, _ = infer_offline.convert_device(model, args, audio, SR, None, encoder, extractor,
                                                torch.full((1, 1), SPK[k], dtype=torch.int64, device=dev), batch_frames=300,
                                                key=KEYS[k], noise_seed=5, units_batch_samples=60000)
        assert waves[k].dtype == np.float64 and waves[k].shape == (alone.numel(),) and np.isfinite(waves[k]).all(), k
        assert float(np.abs(waves[k]).max()) > 1e-3


# ---- gaps between files, the enhancer over all files, the command line on a folder ---------------------------------------------

def test_stitch_of_several_files_leaves_exact_zeros_in_the_gaps(ctx, dev, lib_path):
    """`stitch_plan_many` with odd file totals (813 and 5 samples), an empty file and a file that starts behind a silence: one
    `ddsp_stitch` launch over the table of all files.  Every file's span equals the one-file `stitch` bit for bit, the next
    file starts at the even base, and the samples between - there are some - are exactly 0."""
    import infer_offline
    starts, lengths, block = [[0, 2], [0], [], [1]], [[700, 301], [5], [], [1030]], 256
    rng = np.random.Generator(np.random.PCG64(717))
    pieces = [[torch.from_numpy((0.5 * rng.standard_normal(n)).astype(np.float32)).to(dev) for n in per_file] for per_file in lengths]
    spans, p, fade, total = infer_offline.stitch_plan_many(starts, lengths, block, SR, SR)
    assert spans == [(0, 813), (814, 5), (820, 0), (820, 1286)] and total == 2106 and fade == [0, 188, 0, 0]
    got = ctx.stitch([x for per_file in pieces for x in per_file], p, fade, total)
    covered = torch.zeros(total, dtype=torch.bool, device=got.device)
    for k, (base, n) in enumerate(spans):
        want = infer_offline.stitch(pieces[k], infer_offline.stitch_plan(starts[k], lengths[k], block, SR, SR), device=dev)
        assert torch.equal(got[base:base + n], want), k
        covered[base:base + n] = True
    assert int((~covered).sum()) == 2 and not bool(covered[813]) and not bool(covered[819])
    assert not got[~covered].any() and float(got[814].abs()) > 0 and not got[820:820 + block].any()


def _fixed_enhancer(tmp_path, dev):
    """The small NSF-HiFiGAN of tests/test_gpu_stitch.py from a checkpoint on disk, its random initial phases pinned."""
    import json

    import glue_cases as GC
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


@pytest.mark.parametrize("adaptive_key", [0, 2])
def test_render_many_device_with_the_enhancer_equals_render_device_per_file(dev, lib_path, tmp_path, adaptive_key):
    """The enhancer in ragged groups over the pieces of ALL files (12 000 padded samples: the 11- and 9-frame slices of files 1
    and 0 share a group) against `render_device` per file with the same budgets: another grouping of the enhancer's rows, so
    the file rms error is held to 1e-4, the gate of test_render_with_the_enhancer_in_ragged_groups
    (tests/test_gpu_enhancer_ragged.py).  Whatever lies between the files' spans is exactly 0."""
    import infer_offline
    from ddsp.vocoder import DotDict
    enh = _fixed_enhancer(tmp_path, dev)
    model, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    files, noise = _analysed(dev)
    lengths = [row[2] * HOP for row in files["pieces"]]
    assert any(len({files["pieces"][i][0] for i in g}) > 1 for g in infer_offline.group_segments(lengths, 12000))
    kw = dict(batch_frames=22, enhancer=enh, enhancer_batch_samples=12000, enhancer_adaptive_key=adaptive_key)
    got, spans, sr_o = infer_offline.render_many_device(model, args, files, SPK, noise=noise, **kw)
    want = _per_file_renders(model, args, files, noise, SPK, **kw)
    covered = torch.zeros(got.numel(), dtype=torch.bool, device=got.device)
    end = 0
    for k, (base, total) in enumerate(spans):
        assert base == end + (end & 1) and total == want[k].numel() and float(want[k].abs().max()) > 1e-3, k
        e = rms((got[base:base + total] - want[k]).cpu())
        print(f"enhancer key {adaptive_key} file {k}: {total} samples from {base}, rms error {e:.3e}")
        assert e <= 1e-4, (k, e)
        covered[base:base + total] = True
        end = base + total
    print(f"enhancer key {adaptive_key}: {int((~covered).sum())} gap samples")
    assert got.numel() == end and not got[~covered].any()
    torch.cuda.synchronize()
    infer_offline.hipddsp.context_for(dev).poll_error()


def test_per_file_values_take_one_element_tensors_and_numpy_scalars(dev, lib_path):
    import infer_offline
    from ddsp.vocoder import DotDict
    model, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    files, noise = _analysed(dev)
    a, _, _ = infer_offline.render_many_device(model, args, files, 2, noise=noise, batch_frames=22)
    for spk in (torch.full((1, 1), 2, dtype=torch.int64, device=dev), np.int64(2), [2, 2, 2], torch.tensor([2, 2, 2])):
        b, _, _ = infer_offline.render_many_device(model, args, files, spk, noise=noise, batch_frames=22)
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="one per file"):
        infer_offline.render_many_device(model, args, files, [1, 2], noise=noise, batch_frames=22)


def test_main_run_converts_a_folder(dev, lib_path, encoder, tmp_path):
    """`main.run` with a directory as `-i`: every .wav (sorted) through one `convert_many_device`, written under its name
    into the `-o` directory; the returned tensor is `convert_many_device`'s under the same generator state, the files hold
    the 16-bit samples of their spans.  A file that is no .wav is left alone.  Then the same with `-mix`."""
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
    audios = {"b.wav": _voiced(int(0.9 * SR), 130.0, 9), "a.wav": _voiced(int(0.6 * SR) + 5, 180.0, 10)}
    (tmp_path / "in").mkdir()
    for name, x in audios.items():
        wavfile.write(tmp_path / "in" / name, SR, x)
    (tmp_path / "in" / "notes.txt").write_text("not audio")
    cmd = main.parse_args(["-m", str(tmp_path / "model_0.pt"), "-i", str(tmp_path / "in"), "-o", str(tmp_path / "out"),
                           "-pe", "ac", "-e", "false", "-k", "2", "-id", "3"])
    torch.manual_seed(41)
    result, sr_o = main.run(cmd, units_encoder=encoder, device=dev)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["a.wav", "b.wav"]
    torch.manual_seed(41)
    loaded, args = load_model(str(tmp_path / "model_0.pt"), device=dev)
    want, spans, _ = infer_offline.convert_many_device(
        loaded, args, [torch.from_numpy(audios[n]).to(dev) for n in ("a.wav", "b.wav")], SR, encoder,
        F0_Extractor("ac", SR, HOP, 50.0, 1100.0, device=dev), 3, keys=2.0, batch_frames=4096)
    assert sr_o == SR and torch.equal(result, want)
    host = want.cpu().numpy()
    for name, (base, total) in zip(("a.wav", "b.wav"), spans):
        rate, written = wavfile.read(tmp_path / "out" / name)
        assert rate == SR and written.dtype == np.int16 and int(np.abs(written).max()) > 30
        assert np.array_equal(written, main.pcm16(host[base:base + total])), name
        assert len(written) == (len(audios[name]) // HOP + 1) * HOP
    cmd = main.parse_args(["-m", str(tmp_path / "model_0.pt"), "-i", str(tmp_path / "in"), "-o", str(tmp_path / "mixed"),
                           "-pe", "ac", "-e", "false", "-mix", "{1: 0.5, 3: 0.5}"])
    mixed, _ = main.run(cmd, units_encoder=encoder, device=dev)
    assert mixed.shape == result.shape and bool(torch.isfinite(mixed).all()) and not torch.equal(mixed, result)
    assert sorted(p.name for p in (tmp_path / "mixed").iterdir()) == ["a.wav", "b.wav"]
