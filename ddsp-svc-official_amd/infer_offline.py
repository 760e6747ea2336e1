"""The reference's offline CLI (`main.py:88-174`) restated around the device path.

The reference's `main.py` is broken as shipped (`.astype` on a tensor at :112, key shift applied twice at :105/:120,
SURVEY 0.3), so this module restates what it intends.  `render` takes analysed features and does what happens from there:
per-slice `model(...)[0]`, the volume gate multiplied into the returned signal in place, optional enhancer, silence padding /
cross-fade of slices; with `batch_frames=` the slices are rendered in ragged batches (`model(..., n_frames=)`) instead of
one after the other, and with `enhancer_batch_samples=` they are enhanced in ragged batches too
(`Enhancer.enhance_batch`).  `convert` starts from the raw audio: f0 (`F0_Extractor`), volume and per-slice units
(`Units_Encoder`) on the device, then `render`.  `split` cuts the audio into slices as `main.split` does, with the package's
own `slicer.Slicer` (the reference's silence detector on the device); `convert(..., slices=None, ...)` calls it, or takes
the slice boundaries of any other detector.  `render_device` / `convert_device` are `render` / `convert_batched` with the end
on the device too: one gate launch per ragged group (`ddsp_volume_gate_rows`), one launch for the stitch (`stitch_plan`,
`stitch`: `ddsp_stitch`), the float64 waveform returned as a device tensor; `main.py` is the command line over them.
"""
import numpy as np
import torch

import hipddsp
from sharding import stack_rows
from slicer import Slicer


def cross_fade(a: np.ndarray, b: np.ndarray, idx: int):
    """Linear cross-fade of two host slices (reference `main.py:50-57`); numpy float64 like the reference."""
    out = np.zeros(idx + b.shape[0])
    fade = a.shape[0] - idx
    out[:idx] = a[:idx]
    k = np.linspace(0, 1.0, num=fade, endpoint=True)
    out[idx:a.shape[0]] = (1 - k) * a[idx:] + k * b[:fade]
    out[a.shape[0]:] = b[fade:]
    return out


def volume_mask(volume, threshold_db, block_size):
    """(1, Fr) device volume -> (1, Fr*block) gate, the reference's mask (`main.py:111-116`) as one device kernel."""
    ctx = hipddsp.context_for(volume.device)
    ones = torch.ones(volume.shape[0], volume.shape[1] * block_size, device=volume.device)
    return ctx.volume_gate_(ones, volume, threshold_db, block_size)


def group_segments(lengths, batch_frames):
    """Groups of segment indices for ragged batches: segments sorted by length (longest first, ties in their own order)
    are taken greedily into a group while its padded size, len(group) * longest, stays <= batch_frames; a segment longer
    than batch_frames is a group of its own.  Every index is in exactly one group."""
    groups = []
    for i in sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i)):
        if groups and (len(groups[-1]) + 1) * int(lengths[groups[-1][0]]) <= batch_frames:
            groups[-1].append(i)
        else:
            groups.append([i])
    return groups


def _render_ragged(model, segments, f0, volume, spk_id, spk_mix_dict, noise_seed, batch_frames, block, noise=None):
    """Every segment's signal (1, n * block), in the order of `segments`, from one ragged forward per group.  All groups are
    rendered before the stitch starts, so the whole file's audio is on the device at once (4 bytes per sample)."""
    lengths = [units.size(1) for _, units in segments]
    for (start, _), n in zip(segments, lengths):
        if start < 0 or start + n > f0.shape[1] or start + n > volume.shape[1]:
            raise ValueError(f"render: the segment at frame {start} has {n} frames of units but f0 / volume cover "
                             f"{f0.shape[1]} / {volume.shape[1]} frames of the file")
    rendered = [None] * len(segments)
    for group in group_segments(lengths, batch_frames):
        u, counts = stack_rows([segments[i][1][0] for i in group])
        f, _ = stack_rows([f0[0, segments[i][0]:segments[i][0] + lengths[i]] for i in group])
        v, _ = stack_rows([volume[0, segments[i][0]:segments[i][0] + lengths[i]] for i in group])
        kw = {} if noise_seed is None else {"noise_seed": noise_seed + min(segments[i][0] for i in group)}
        if noise is not None:
            kw["noise"] = stack_rows([noise[i].reshape(-1) for i in group])[0]
        signal = model(u, f, v, spk_id=spk_id, spk_mix_dict=spk_mix_dict, n_frames=counts, **kw)[0]
        for j, i in enumerate(group):
            rendered[i] = signal[j:j + 1, :counts[j] * block].clone()
    return rendered


def _encode_ragged(units_encoder, pieces, sample_rate, hop_size, units_batch_samples):
    """pieces: [(start_frame, audio (1, n))] -> [(start_frame, units (1, int(n // hop_size) + 1, n_unit))] in the same order,
    from one ragged `Units_Encoder.encode` per group of `group_segments` over the sample lengths."""
    lengths = [seg.shape[-1] for _, seg in pieces]
    out = [None] * len(pieces)
    for group in group_segments(lengths, int(units_batch_samples)):
        wav, counts = stack_rows([pieces[i][1][0] for i in group])
        units = units_encoder.encode(wav, sample_rate, hop_size, n_samples=counts)
        for j, i in enumerate(group):
            out[i] = (pieces[i][0], units[j:j + 1, :int(counts[j] // hop_size) + 1].clone())
    return out


def _enhance_ragged(enhancer, gated, segments, f0, sr, block, adaptive_key, enhancer_batch_samples):
    """Every gated slice (1, n * block) enhanced, in the order of `segments`, from one `Enhancer.enhance_batch` per group of
    `group_segments` over the sample lengths, each row with its own f0 slice -> ([(1, n_out)], enhancer sample rate)."""
    lengths = [g.shape[-1] for g in gated]
    out, sr_o = [None] * len(gated), sr
    for group in group_segments(lengths, int(enhancer_batch_samples)):
        wav, counts = stack_rows([gated[i][0] for i in group])
        tracks, n_f0 = stack_rows([f0[0, segments[i][0]:segments[i][0] + segments[i][1].size(1), 0] for i in group])
        got, sr_o, n_out = enhancer.enhance_batch(wav, sr, tracks[:, :, None], block, counts, adaptive_key=adaptive_key, n_f0=n_f0)
        for j, i in enumerate(group):
            out[i] = got[j:j + 1, :n_out[j]]
    return out, sr_o


@torch.no_grad()
def render(model, args, segments, f0, volume, spk_id, spk_mix_dict=None, threshold_db=-60, enhancer=None,
           enhancer_adaptive_key=0, noise_seed=None, batch_frames=None, noise=None, enhancer_batch_samples=None):
    """segments: list of (start_frame, units (1, Fr_seg, n_unit)) as `main.py:143-151` produces them;
    f0 (1, Fr, 1), volume (1, Fr) cover the whole file.  Returns (float64 numpy waveform, sample rate).
    batch_frames: None renders slice after slice at batch 1; a number renders the slices in ragged batches of at most that
    many padded frames (`group_segments`), one forward per group, each slice as if rendered alone; gate, enhancer, silence
    and cross-fade then run per slice in the original order, so the file is stitched the same way.
    noise: a list with one (n * block,) U[0,1) draw per segment that stands where the model draws its noise (parity runs).
    enhancer_batch_samples: None enhances slice after slice; a number enhances the gated slices in ragged groups
    (`group_segments` over their sample lengths, at most that many padded samples per group, one `Enhancer.enhance_batch`
    each with every row's own f0 slice), every slice as if enhanced alone; the gate comes first and the stitch after, as
    without it.  All slices are then on the device at once."""
    block = int(args.data.block_size)
    sr = int(args.data.sampling_rate)
    ctx = hipddsp.context_for(f0.device)
    result = np.zeros(0)
    current = 0
    sr_o = sr
    rendered = None if batch_frames is None else \
        _render_ragged(model, segments, f0, volume, spk_id, spk_mix_dict, noise_seed, int(batch_frames), block, noise)

    def gated_slice(i):
        start, units = segments[i]
        n = units.size(1)
        seg_f0 = f0[:, start:start + n, :]
        seg_vol = volume[:, start:start + n]
        if rendered is not None:
            out = rendered[i]
        else:
            kw = {} if noise_seed is None else {"noise_seed": noise_seed + start}
            if noise is not None:
                kw["noise"] = noise[i].reshape(1, -1)
            out = model(units, seg_f0, seg_vol, spk_id=spk_id, spk_mix_dict=spk_mix_dict, **kw)[0]
        # the gate of the WHOLE file sliced to this segment (main.py:159): dilation sees the neighbours
        gate = volume_mask(volume, threshold_db, block)[:, start * block:(start + n) * block]
        out *= gate
        return out, seg_f0

    enhanced = None
    if enhancer is not None and enhancer_batch_samples is not None and segments:
        enhanced, sr_o = _enhance_ragged(enhancer, [gated_slice(i)[0] for i in range(len(segments))], segments, f0, sr, block,
                                         enhancer_adaptive_key, enhancer_batch_samples)
    for i, (start, units) in enumerate(segments):
        if enhanced is not None:
            out = enhanced[i]
        else:
            out, seg_f0 = gated_slice(i)
            if enhancer is not None:
                out, sr_o = enhancer.enhance(out, sr, seg_f0, block, adaptive_key=enhancer_adaptive_key)
        out = out.squeeze().cpu().numpy()
        silent = round(start * block * sr_o / sr) - current
        if silent >= 0:
            result = np.append(result, np.zeros(silent))
            result = np.append(result, out)
        else:
            result = cross_fade(result, out, current + silent)
        current = current + silent + len(out)
    return result, sr_o


def stitch_plan(starts, lengths, block, sr, sr_o):
    """Where the stitch of `main.py:165-173` puts every piece -> (p, fade, total): piece i, rendered from start frame
    starts[i] with lengths[i] samples at the output rate sr_o, begins at output sample p[i] = round(starts[i] * block * sr_o /
    sr) (Python's `round` on that float expression, as the reference writes it), cross-fades its first fade[i] = max(0, end
    of piece i-1 - p[i]) samples (`cross_fade`) and ends at p[i] + lengths[i]; total is the last end (0 without pieces).
    Raises ValueError naming the piece when it has no samples, starts before its predecessor (`main.split` yields ascending
    frames), or is shorter than its fade (the reference's `cross_fade` fails to broadcast there).  Host code only."""
    if len(starts) != len(lengths):
        raise ValueError(f"stitch_plan: {len(starts)} start frames for {len(lengths)} pieces")
    p, fade, cur = [], [], 0
    for i, (start, n) in enumerate(zip(starts, lengths)):
        start, n = int(start), int(n)
        at = round(start * block * sr_o / sr)
        if n < 1:
            raise ValueError(f"stitch_plan: piece {i} (start frame {start}) has no samples")
        if p and at < p[-1]:
            raise ValueError(f"stitch_plan: piece {i} starts at output sample {at}, before piece {i - 1} at {p[-1]}: the "
                             "start frames must ascend")
        f = max(0, cur - at)
        if n < f:
            raise ValueError(f"stitch_plan: piece {i} has {n} samples but overlaps the result so far by {f}: a piece must "
                             "be at least as long as its cross-fade")
        p.append(at)
        fade.append(f)
        cur = at + n
    return p, fade, cur


def stitch(pieces, plan, device=None):
    """pieces: the rendered slices, fp32 device tensors of any shape holding lengths[i] contiguous samples (rows of a padded
    group tensor are fine: nothing is packed); plan: `stitch_plan` of their start frames and lengths -> the stitched file as
    an fp64 device tensor (total,), equal to the reference's host loop (`np.append` / `cross_fade` per slice) bit for bit,
    from one `ddsp_stitch` launch.  An empty list gives a tensor of length 0 (on `device`, the current HIP device if None)."""
    p, fade, total = plan
    if not (len(pieces) == len(p) == len(fade)):
        raise ValueError(f"stitch: {len(pieces)} pieces for a plan of {len(p)}")
    cur = 0
    for i, x in enumerate(pieces):   # the plan is the plan of THESE lengths
        if x.numel() < 1 or fade[i] != max(0, cur - p[i]) or x.numel() < fade[i]:
            raise ValueError(f"stitch: piece {i} has {x.numel()} samples, which is not what the plan was made for")
        cur = p[i] + x.numel()
    if cur != total:
        raise ValueError(f"stitch: the pieces end at sample {cur}, the plan at {total}")
    if not pieces:
        return torch.zeros(0, dtype=torch.float64, device="cuda" if device is None else device)
    return hipddsp.context_for(pieces[0].device).stitch(pieces, p, fade, total)


@torch.no_grad()
def render_device(model, args, segments, f0, volume, spk_id, spk_mix_dict=None, threshold_db=-60, enhancer=None,
                  enhancer_adaptive_key=0, noise_seed=None, batch_frames=None, noise=None, enhancer_batch_samples=None):
    """`render` with its keywords, the result left on the device -> (fp64 device tensor (total,), sample rate), equal to
    `render`'s array.  Ragged groups through `model(..., n_frames=)`, ONE `ddsp_volume_gate_rows` per group on the group's
    padded signal (no gate per slice, no whole-file `ones`), `_enhance_ragged` when there is an enhancer, one `stitch` of the
    rows where they lie.  `batch_frames=None` / `enhancer_batch_samples=None`: one slice per group.  Nothing is read back
    between the first forward and the returned tensor beyond what `Enhancer.enhance_batch` itself reads."""
    block = int(args.data.block_size)
    sr = int(args.data.sampling_rate)
    ctx = hipddsp.context_for(f0.device)
    lengths = [units.size(1) for _, units in segments]
    for (start, _), n in zip(segments, lengths):
        if start < 0 or start + n > f0.shape[1] or start + n > volume.shape[1]:
            raise ValueError(f"render_device: the segment at frame {start} has {n} frames of units but f0 / volume cover "
                             f"{f0.shape[1]} / {volume.shape[1]} frames of the file")
    pieces = [None] * len(segments)
    for group in group_segments(lengths, 0 if batch_frames is None else int(batch_frames)):
        starts = [segments[i][0] for i in group]
        u, counts = stack_rows([segments[i][1][0] for i in group])
        f, _ = stack_rows([f0[0, s:s + n] for s, n in zip(starts, counts)])
        v, _ = stack_rows([volume[0, s:s + n] for s, n in zip(starts, counts)])
        kw = {} if noise_seed is None else {"noise_seed": noise_seed + min(starts)}
        if noise is not None:
            kw["noise"] = stack_rows([noise[i].reshape(-1) for i in group])[0]
        signal = model(u, f, v, spk_id=spk_id, spk_mix_dict=spk_mix_dict, n_frames=counts, **kw)[0].contiguous()
        ctx.volume_gate_rows_(signal, volume[0], ctx.ragged_counts(starts), ctx.ragged_counts(counts), threshold_db, block)
        for j, i in enumerate(group):
            pieces[i] = signal[j:j + 1, :counts[j] * block]
    sr_o = sr
    if enhancer is not None and segments:
        pieces, sr_o = _enhance_ragged(enhancer, pieces, segments, f0, sr, block, enhancer_adaptive_key,
                                       0 if enhancer_batch_samples is None else enhancer_batch_samples)
    plan = stitch_plan([start for start, _ in segments], [x.shape[-1] for x in pieces], block, sr, sr_o)
    return stitch(pieces, plan, device=f0.device), sr_o


def split(audio, sample_rate, hop_size, db_thresh=-40, min_len=5000):
    """The slicing of `main.split` (main.py:34-40): audio (T,) numpy array or tensor at `sample_rate` -> the list of
    (start_sample, end_sample) of every chunk `Slicer(sr=sample_rate, threshold=db_thresh, min_length=min_len)` tags with
    start != end - the silence chunks too: `main.split` does not look at the flag.  One read-back (chunk table and count).
    The snapping to whole frames of `hop_size` (main.py:41-46) is `convert`'s."""
    rows = Slicer(sr=sample_rate, threshold=db_thresh, min_length=min_len).chunk_rows(audio)
    return [(int(a), int(b)) for a, b, _ in rows if a != b]


@torch.no_grad()
def convert(model, args, audio, sample_rate, slices, units_encoder, f0_extractor, spk_id, key=0, spk_mix_dict=None,
            threshold_db=-60, enhancer=None, enhancer_adaptive_key=0, noise_seed=None):
    """`main.py:88-174` from the raw audio: audio (T,) numpy array or device tensor at `sample_rate`; `slices` a list of
    (start_sample, end_sample) as the reference's `Slicer` tags them (`split_time`) - what `split` returns, or the ranges of
    any other silence detector - or None: `split(audio, sample_rate, hop_size)` with `main.py`'s defaults.  f0 of the whole file (uv_interp on) shifted by `key`
    semitones ONCE (the reference applies the shift twice), volume of the whole file at
    `hop_size = block_size * sample_rate / sampling_rate`, then per slice, snapped to whole frames as `main.split` does
    (main.py:41-46: start_frame = int(start // hop_size), end_frame = int(end // hop_size), audio[int(start_frame *
    hop_size) : int(end_frame * hop_size)], empty slices dropped), the units of that slice's audio (main.py:148-151), then
    `render`.  `units_encoder` / `f0_extractor`: `ddsp.vocoder.Units_Encoder` / `F0_Extractor` built for `sample_rate` and
    that hop (ValueError otherwise).  Returns (float64 numpy waveform, sample rate).
    `convert_batched` is the same call with the slices rendered in ragged batches."""
    return convert_batched(model, args, audio, sample_rate, slices, units_encoder, f0_extractor, spk_id, None, key=key,
                           spk_mix_dict=spk_mix_dict, threshold_db=threshold_db, enhancer=enhancer,
                           enhancer_adaptive_key=enhancer_adaptive_key, noise_seed=noise_seed)


@torch.no_grad()
def convert_batched(model, args, audio, sample_rate, slices, units_encoder, f0_extractor, spk_id, batch_frames, key=0,
                    spk_mix_dict=None, threshold_db=-60, enhancer=None, enhancer_adaptive_key=0, noise_seed=None,
                    enhancer_batch_samples=None, units_batch_samples=None):
    """`convert` with `render`'s `batch_frames`: the slices are rendered in ragged batches of at most that many padded frames
    (None: slice after slice, which is `convert`).  `units_batch_samples`: None encodes the units slice by slice; a number
    encodes them in ragged groups too (`Units_Encoder.encode(..., n_samples=)`), `group_segments` over the slices' sample
    lengths with at most that many padded samples (at `sample_rate`) per group, every slice as if encoded alone.
    `enhancer_batch_samples`: `render`'s keyword of that name - None enhances slice after slice, a number in ragged groups of
    at most that many padded samples (at the model's rate); it stands before `units_batch_samples`, which
    tests/test_hubert_ragged_host.py pins as the last parameter.  (A function of its own and not a keyword of `convert`:
    tests/test_stream_audio_host.py pins `convert`'s parameter list.)"""
    segments, f0, volume = _analyse(args, audio, sample_rate, slices, units_encoder, f0_extractor, key, units_batch_samples)
    return render(model, args, segments, f0, volume, spk_id, spk_mix_dict=spk_mix_dict, threshold_db=threshold_db,
                  enhancer=enhancer, enhancer_adaptive_key=enhancer_adaptive_key, noise_seed=noise_seed, batch_frames=batch_frames,
                  enhancer_batch_samples=enhancer_batch_samples)


@torch.no_grad()
def convert_device(model, args, audio, sample_rate, slices, units_encoder, f0_extractor, spk_id, batch_frames=None, key=0,
                   spk_mix_dict=None, threshold_db=-60, enhancer=None, enhancer_adaptive_key=0, noise_seed=None,
                   enhancer_batch_samples=None, units_batch_samples=None):
    """`convert_batched` ending in `render_device`: the same analysis, then ragged rendering, one gate launch per group, the
    ragged enhancer and one stitch launch -> (fp64 device tensor (total,), sample rate), equal to `convert_batched`'s array.
    One `.cpu()` of the result is the file's only read-back behind the slicer's chunk table."""
    segments, f0, volume = _analyse(args, audio, sample_rate, slices, units_encoder, f0_extractor, key, units_batch_samples)
    return render_device(model, args, segments, f0, volume, spk_id, spk_mix_dict=spk_mix_dict, threshold_db=threshold_db,
                         enhancer=enhancer, enhancer_adaptive_key=enhancer_adaptive_key, noise_seed=noise_seed,
                         batch_frames=batch_frames, enhancer_batch_samples=enhancer_batch_samples)


def _analyse(args, audio, sample_rate, slices, units_encoder, f0_extractor, key, units_batch_samples):
    """The part of `convert` in front of the rendering -> (segments [(start_frame, units (1, Fr_seg, n_unit))], f0 (1, Fr, 1)
    shifted by `key`, volume (1, Fr)), all on the device."""
    hop_size = int(args.data.block_size) * sample_rate / int(args.data.sampling_rate)
    if f0_extractor.sample_rate != sample_rate or f0_extractor.hop_size != hop_size:
        raise ValueError(f"convert: the f0 extractor works at {f0_extractor.sample_rate} Hz with hop {f0_extractor.hop_size}; "
                         f"the audio is at {sample_rate} Hz with hop {hop_size}")
    if isinstance(audio, np.ndarray):
        audio = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32))
    dev = audio.device if audio.is_cuda else torch.device(f0_extractor.device)
    x = audio.reshape(-1).to(dev, torch.float32)
    f0 = f0_extractor.extract(x, uv_interp=True)[None, :, None]
    if key != 0:
        f0 = f0 * 2 ** (float(key) / 12)
    volume = hipddsp.context_for(dev).volume_extract(x[None], hop_size)
    if slices is None:
        slices = split(x, sample_rate, hop_size)
    segments = []
    for start, end in slices:
        start_frame, end_frame = int(int(start) // hop_size), int(int(end) // hop_size)
        if end_frame > start_frame:
            seg = x[None, int(start_frame * hop_size):int(end_frame * hop_size)]
            segments.append((start_frame, seg if units_batch_samples is not None else
                             units_encoder.encode(seg, sample_rate, hop_size)))
    if units_batch_samples is not None:
        segments = _encode_ragged(units_encoder, segments, sample_rate, hop_size, units_batch_samples)
    return segments, f0, volume
