"""The reference's offline CLI (`main.py:88-174`) restated around the device path.

The reference's `main.py` is broken as shipped (`.astype` on a tensor at :112, key shift applied twice at :105/:120,
SURVEY 0.3), so this module restates what it intends.  `render` takes analysed features and does what happens from there:
per-slice `model(...)[0]`, the volume gate multiplied into the returned signal in place, optional enhancer, silence padding /
cross-fade of slices; with `batch_frames=` the slices are rendered in ragged batches (`model(..., n_frames=)`) instead of
one after the other, and with `enhancer_batch_samples=` they are enhanced in ragged batches too
(`Enhancer.enhance_batch`).  `convert` starts from the raw audio: f0 (`F0_Extractor`), volume and per-slice units
(`Units_Encoder`) on the device, then `render`.  `split` cuts the audio into slices as `main.split` does, with the package's
own `slicer.Slicer` (the reference's silence detector on the device); `convert(..., slices=None, ...)` calls it, or takes
the slice boundaries of any other detector: the reference-shaped statement the device path is held to sample for sample.
The device path is ONE body over a LIST of files (`_analyse_files`, `_render_files`): one analysis of all files, ragged groups
over the slices of all files (rows formed by `ddsp_pieces_gather`, gated by `ddsp_volume_gate_files`), one stitch of every
file into one fp64 device tensor (`stitch_plan_many`, `ddsp_stitch`), one read-back: `analyse_many` / `render_many_device` /
`convert_many_device` / `convert_many`.  `render_device` / `convert_device` - `render` / `convert_batched` with the end on the
device - are that body on a list of one file, which is its own batch and keeps `render`'s seed and speaker rules.
The same body renders JOBS (`convert_many_device(jobs=, models=)`, `render_jobs_device`, `job_table`): a job is a file, a model, a
speaker or mix and a key; the files are analysed once whatever the number of jobs, a row names its file for the source and its
job for key, speaker and output span, and the groups are formed model by model.  What a job may carry beyond that - timelines,
formant shift, pitch correction, unit retrieval, envelope mix - and the `Job` record itself live in `controls`, whose names are
importable from here as well.  `to_pcm16` turns the result into 16-bit PCM on the device (`ddsp_pcm16`), so the read-back is 2
bytes per sample.
"""
import numbers

import numpy as np
import torch

import hipddsp
from controls import (MAX_FORMANT, NOTE_NAMES, SCALES, EnvelopeMix, FormantTimeline, Job, KeyTimeline, PitchTune,  # noqa: F401
                      SpeakerTimeline, UnitIndex, UnitIndexBank, check_job_index, envelope_tables, formant_tables, index_tables,
                      job_envelopes, job_formants, job_indices, job_tunes, key_tables, pitch_class, timeline_tables, tune_tables)
from ddsp.analysis import MODEL_FIELDS, _model_field, check_units_width
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
    from one ragged `Units_Encoder.encode` per group of `group_segments` over the sample lengths.  The torch-slice statement
    of what `_analyse_files` does with `ddsp_pieces_gather` rows (tests/test_hubert_ragged_host.py holds its grouping)."""
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
    `group_segments` over the sample lengths, each row with its own f0 slice -> ([(1, n_out)], enhancer sample rate).
    Serves `render` alone: the device path enhances with `_enhance_many`."""
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


SLICER_DB_THRESH, SLICER_MIN_LEN = -40, 5000      # `main.py`'s slicer settings: `split`'s defaults and `slices=None`


def split(audio, sample_rate, hop_size, db_thresh=SLICER_DB_THRESH, min_len=SLICER_MIN_LEN):
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
    check_units_width("convert", units_encoder, model)
    segments, f0, volume = _analyse(args, audio, sample_rate, slices, units_encoder, f0_extractor, key, units_batch_samples)
    return render(model, args, segments, f0, volume, spk_id, spk_mix_dict=spk_mix_dict, threshold_db=threshold_db,
                  enhancer=enhancer, enhancer_adaptive_key=enhancer_adaptive_key, noise_seed=noise_seed, batch_frames=batch_frames,
                  enhancer_batch_samples=enhancer_batch_samples)


# ---- the device path: a list of files in one call, ragged groups across files ---------------------------------------------

def piece_table(slices_per_file, hop_size):
    """The pieces of several files as `ddsp_pieces_gather` takes them: `slices_per_file[k]` is file k's list of (start_sample,
    end_sample) -> the list of (file, start_frame, n_frames, start_sample, n_samples), files in order and every file's slices in
    theirs.  The snapping is `main.split`'s (main.py:41-46), formed here on the host because `hop_size` may be fractional:
    start_frame = int(start // hop_size), end_frame = int(end // hop_size), start_sample = int(start_frame * hop_size),
    n_samples = int(end_frame * hop_size) - start_sample; a slice with end_frame == start_frame is dropped.  n_frames =
    int(n_samples // hop_size) + 1 is the number of unit frames `Units_Encoder.encode` gives the slice, which is what the slice
    takes of its file's f0 and volume."""
    rows = []
    for k, slices in enumerate(slices_per_file):
        for start, end in slices:
            start_frame, end_frame = int(int(start) // hop_size), int(int(end) // hop_size)
            if end_frame > start_frame:
                start_sample = int(start_frame * hop_size)
                n_samples = int(end_frame * hop_size) - start_sample
                rows.append((k, start_frame, int(n_samples // hop_size) + 1, start_sample, n_samples))
    return rows


def stitch_plan_many(starts_per_file, lengths_per_file, block, sr, sr_o):
    """`stitch_plan` for several files laid one after the other in ONE output -> (spans, p, fade, total): spans[k] = (base,
    total) of file k, its samples out[base:base + total]; p, fade the table of all pieces, files in order, for one `ddsp_stitch`
    launch; total the end of the last file.  File k's base is the end of the files before it rounded up to a multiple of 2
    samples (16 bytes of fp64: every file starts where the kernel's stores are aligned), its pieces sit at base + their own p
    with their own fades - 0 at a file's first piece, so nothing fades across files - and the gap the rounding leaves is covered
    by no piece: exact zeros.  A file without pieces has total 0.  Raises `stitch_plan`'s ValueErrors, naming the file too."""
    if len(starts_per_file) != len(lengths_per_file):
        raise ValueError(f"stitch_plan_many: start frames of {len(starts_per_file)} files, lengths of {len(lengths_per_file)}")
    spans, p, fade, end = [], [], [], 0
    for k, (starts, lengths) in enumerate(zip(starts_per_file, lengths_per_file)):
        try:
            pk, fk, total = stitch_plan(starts, lengths, block, sr, sr_o)
        except ValueError as e:
            raise ValueError(f"stitch_plan_many: file {k}: {e}") from None
        base = end + (end & 1)
        spans.append((base, total))
        p.extend(base + at for at in pk)
        fade.extend(fk)
        end = base + total
    return spans, p, fade, end


def group_pieces(pieces, budget, by_samples=False):
    """`group_segments` over the pieces of ALL files (`piece_table` rows), by their frame counts or (by_samples) their sample
    counts -> groups of indices into `pieces`; every (file, slice) is in exactly one group and a group may hold rows of
    several files."""
    return group_segments([row[4 if by_samples else 2] for row in pieces], budget)


def _check_formant(j, formant, model):
    if isinstance(formant, FormantTimeline):
        try:
            formant.frames(_model_field(model, "sampling_rate"), _model_field(model, "block_size"))
        except ValueError as e:
            raise ValueError(f"job_table: job {j}: {e}") from None
    elif formant is not None:
        if isinstance(formant, KeyTimeline):
            raise ValueError(f"job_table: job {j}: formant must be a number of semitones or a FormantTimeline, got a KeyTimeline")
        try:
            hipddsp.formant_factor(formant, MAX_FORMANT)
        except ValueError as e:
            raise ValueError(f"job_table: job {j}: {e}") from None


def job_table(pieces, n_files, jobs, models, n_indices=None):
    """The tables of a conversion of `jobs` over analysed files, made and checked on the host (nothing is launched).  pieces:
    `piece_table` rows of the `n_files` files; jobs: a sequence of (file, model_index, spk, key) - spk a 1-based speaker id, a
    mix dict {id: weight} or a `SpeakerTimeline` (a voice that changes over the file; it stands in `speakers` as it is, its ids
    checked against the job's model and its points against that model's frame rate), key in semitones, a number or a `KeyTimeline`
    (a key that moves over the file; its points are checked against the job's model's frame rate); models: the synthesisers, which share the analysis and the stitch and so agree in
    sampling rate, block size, unit width and device.  -> a dict:
      rows          [(file, start_frame, n_frames, start_sample, n_samples, job)]: job after job, each with ALL pieces of its file
                    in the file's order - the SAME source columns for every job over that file, which `ddsp_pieces_gather_jobs`
                    reads in place; the sixth column names whose key factor (and speaker, and output span) the row takes;
      piece_of_row  for every row, its index in `pieces` (whose units it takes);
      model_of_job, speakers (an int or a dict per job), key_factor (2 ** (key / 12) per job, Python floats; None for a job
                    whose key is a `KeyTimeline`);
      keys          every job's key as `key_tables` takes it: a float, or the `KeyTimeline` as it is;
      starts_per_job  the start frames of every job's rows, as `stitch_plan_many` takes them with jobs in the place of files.
    A job may carry a fifth entry, its FORMANT shift: a number of semitones (|s| <= 24), a `FormantTimeline` or None.  It is
    checked here and stands in no table of the dict: `job_formants(jobs)` lists it, `formant_tables` makes its breakpoints.
    A sixth entry is its PITCH CORRECTION, a `PitchTune` or None (the formant may then be None too): `job_tunes(jobs)` lists
    it, `tune_tables` makes its settings.
    A seventh entry is its UNIT RETRIEVAL, (index_number, ratio) or None (formant and tune may then be None too): the index of a
    `UnitIndexBank` and the blend ratio in [0, 1]; `job_indices(jobs)` lists it, `index_tables` makes its rows.  n_indices: the
    size of the call's bank where it is known (an index number at or past it is refused).
    An eighth entry is its ENVELOPE MIX, an `EnvelopeMix` (the three in front may be None; `Job.of` states what the tuple form
    takes in that place, and `EnvelopeMix(1.0)` is a job that has it switched off): `job_envelopes(jobs)` lists it, None for a
    job without one, `envelope_tables` makes its rates; the jobs of one call share its `hop_seconds` and `frames` and differ in
    `rate`.
    A job may as well be a `Job` record, which names these entries (file, model, spk, key, formant, tune, index, envelope):
    every job is read through `Job.of`, once, and a list of records is taken as it is.
    ValueError - before any launch - names the first model that disagrees with models[0], a job that is no 4- to 8-tuple (all
    jobs are read before any value is checked), two envelopes of different hop or window, an index entry that is no (int >= 0,
    ratio in [0, 1]), a tune that is no `PitchTune`, an envelope that is no `EnvelopeMix`, a file or model index out of range,
    a speaker id outside [1, n_spk] of the JOB's model, a mix with no or too many speakers, or a formant shift that is no
    finite number within +-24 semitones and no `FormantTimeline` that fits the model's frame rate."""
    models = list(models) if isinstance(models, (tuple, list)) else []
    if not models:
        raise ValueError("job_table: models must be a non-empty list of synthesisers")
    for k, m in enumerate(models[1:], 1):
        for field in MODEL_FIELDS:
            a, b = _model_field(models[0], field), _model_field(m, field)
            if a != b:
                raise ValueError(f"job_table: models[{k}].{field} is {b}, models[0].{field} is {a}: the models of one call agree "
                                 f"in {', '.join(MODEL_FIELDS)}")
    jobs = [Job.of(j, job) for j, job in enumerate(jobs)]
    try:                                 # (the jobs of a call share the envelope's hop and window)
        envelope_tables([job.envelope if isinstance(job.envelope, EnvelopeMix) else None for job in jobs])
    except ValueError as e:
        raise ValueError(f"job_table: {e}") from None
    per_file = [[i for i, row in enumerate(pieces) if row[0] == k] for k in range(int(n_files))]
    table = {"rows": [], "piece_of_row": [], "model_of_job": [], "speakers": [], "key_factor": [], "starts_per_job": [],
             "keys": []}
    for j, job in enumerate(jobs):
        check_job_index(f"job_table: job {j}", job.index, n_indices)
        if not (job.tune is None or isinstance(job.tune, PitchTune)):                # (a record's: `Job.of` checks a tuple's)
            raise ValueError(f"job_table: job {j}: tune must be a PitchTune or None, got {job.tune!r}")
        if not (job.envelope is None or isinstance(job.envelope, EnvelopeMix)):
            raise ValueError(f"job_table: job {j}: envelope must be an EnvelopeMix, got {job.envelope!r}")
        file, m, spk, key = job.file, job.model, job.spk, job.key
        if not (isinstance(file, numbers.Integral) and 0 <= file < int(n_files)):
            raise ValueError(f"job_table: job {j}: file {file!r} is outside the {int(n_files)} files of the call")
        if not (isinstance(m, numbers.Integral) and 0 <= m < len(models)):
            raise ValueError(f"job_table: job {j}: model index {m!r} is outside the {len(models)} models of the call")
        n_spk = int(models[m].unit2ctrl.n_spk)
        if isinstance(spk, SpeakerTimeline):
            ids = spk.ids               # (at most MAX_MIX: the timeline checked that)
            try:
                spk.frames(_model_field(models[m], "sampling_rate"), _model_field(models[m], "block_size"))
            except ValueError as e:
                raise ValueError(f"job_table: job {j}: {e}") from None
        elif isinstance(spk, dict):
            if not 1 <= len(spk) <= hipddsp.MAX_MIX:
                raise ValueError(f"job_table: job {j}: a speaker mix holds 1 to {hipddsp.MAX_MIX} ids, got {len(spk)}")
            ids = list(spk)
            spk = {int(i): float(w) for i, w in spk.items()}
        else:
            if not isinstance(spk, numbers.Integral):
                raise ValueError(f"job_table: job {j}: spk must be a speaker id or a mix dict, got {spk!r}")
            ids = [spk]
            spk = int(spk)
        for i in ids:
            if not (isinstance(i, numbers.Integral) and 1 <= i <= n_spk):
                raise ValueError(f"job_table: job {j}: speaker id {i!r} is outside [1, {n_spk}] of models[{m}]")
        if isinstance(key, FormantTimeline):
            raise ValueError(f"job_table: job {j}: key must be a number of semitones or a KeyTimeline, got a FormantTimeline")
        _check_formant(j, job.formant, models[m])
        if isinstance(key, KeyTimeline):
            try:
                key.frames(_model_field(models[m], "sampling_rate"), _model_field(models[m], "block_size"))
            except ValueError as e:
                raise ValueError(f"job_table: job {j}: {e}") from None
        elif not isinstance(key, numbers.Real):
            raise ValueError(f"job_table: job {j}: key must be a number of semitones or a KeyTimeline, got {key!r}")
        table["rows"].extend(tuple(pieces[i]) + (j,) for i in per_file[file])
        table["piece_of_row"].extend(per_file[file])
        table["starts_per_job"].append([pieces[i][1] for i in per_file[file]])
        table["model_of_job"].append(int(m))
        table["speakers"].append(spk)
        table["key_factor"].append(None if isinstance(key, KeyTimeline) else 2 ** (float(key) / 12))
        table["keys"].append(key if isinstance(key, KeyTimeline) else float(key))
    return table


def job_groups(table, n_models, batch_frames):
    """The ragged render groups of `job_table`'s rows -> [(model_index, [row indices])]: model after model in `models` order,
    `group_segments` over the frame counts of the rows of that model's jobs (a model without jobs has no group).  The position
    in this list is the group's number g of the `noise_seed` rule (seed + g * 2**32)."""
    out = []
    for m in range(int(n_models)):
        idx = [i for i, row in enumerate(table["rows"]) if table["model_of_job"][row[5]] == m]
        out.extend((m, [idx[i] for i in group]) for group in group_segments([table["rows"][i][2] for i in idx], batch_frames))
    return out


def _upload_pieces(ctx, files, groups, rows=None):
    """The piece table of `files` in the order the groups take it -> (table (P, 5) int32 device, its transpose (5, P),
    [(first, last + 1)] of every group): a group's rows, and each of its columns, are contiguous views.  The upload is kept in
    `files` and serves every later stage that asks for the same rows: the order of `group_segments` is the sort by length
    whatever the budget, so the units (whole hops of samples), the forwards and the enhancer of one call share one upload.
    A blocking copy in front of a stage would make the device wait while the host issues that stage's launches.
    rows: the rows the groups index in place of `files['pieces']` - `job_table`'s, of six columns."""
    width = 5 if rows is None else 6
    rows = [(files["pieces"] if rows is None else rows)[i] for group in groups for i in group]
    if files.get("table_rows") != rows:
        table = torch.tensor(rows, dtype=torch.int32).reshape(-1, width).to(ctx.device)
        files.update(table_rows=rows, table=table, table_cols=table.t().contiguous())
    bounds, at = [], 0
    for group in groups:
        bounds.append((at, at + len(group)))
        at += len(group)
    return files["table"], files["table_cols"], bounds


def _per_file(value, F, what):
    """One value (a number, a numpy scalar, a tensor of one element such as `render_device`'s spk_id (1, 1)) or one per file
    -> the list of F values."""
    if isinstance(value, (torch.Tensor, np.ndarray)):
        value = value.reshape(-1).tolist()
        if len(value) == 1:
            value = value[0]
    if isinstance(value, numbers.Real):
        return [value] * F
    value = list(value)
    if len(value) != F:
        raise ValueError(f"{what}: one value or one per file ({F}), got {len(value)}")
    return value


@torch.no_grad()
def analyse_many(args, audios, sample_rate, slices, units_encoder, f0_extractor, keys=0, units_batch_samples=None):
    """The analysis of a list of files at one `sample_rate`: `audios[k]` a numpy array or tensor (T_k,).  ONE ragged
    `F0_Extractor.extract(..., uv_interp=True, n_samples=)`, ONE ragged volume and - `slices` None - ONE ragged slicer call with
    one read-back of the chunk tables cover all files (otherwise `slices[k]` is file k's list of (start_sample, end_sample));
    the units of all slices of all files are encoded in `group_segments` groups over the global list of slices
    (`units_batch_samples` padded samples per group; None: a slice per group), each group's audio rows formed by one
    `ddsp_pieces_gather`.  `keys`: semitones, one number or one per file.  The ragged volume needs an integral hop
    (`block_size * sample_rate / sampling_rate`): ValueError otherwise, before anything is launched.
    -> the dict `render_many_device` takes: audio (F, T_max), f0 (F, Fr_max) NOT yet shifted, volume (F, Fr_max), key_factor
    (F,) fp32 = 2 ** (key / 12), n_samples / n_frames (lists) and n_samples_dev / n_frames_dev, pieces (`piece_table`), units
    (one (1, n_frames, n_unit) tensor per piece), hop_size, sample_rate, device.  `file_features` gives one file's part in
    `_analyse`'s form."""
    hop_size = int(args.data.block_size) * sample_rate / int(args.data.sampling_rate)
    if not float(hop_size).is_integer():
        raise ValueError(f"analyse_many: the ragged volume (n_samples=) needs an integral hop, but block_size * sample_rate / "
                         f"sampling_rate = {hop_size}; resample the files to the model's rate first")
    return _analyse_files(args, audios, sample_rate, slices, units_encoder, f0_extractor, keys, units_batch_samples)


def _analyse(args, audio, sample_rate, slices, units_encoder, f0_extractor, key, units_batch_samples):
    """The part of `convert` in front of the rendering -> (segments [(start_frame, units (1, Fr_seg, n_unit))], f0 (1, Fr, 1)
    shifted by `key`, volume (1, Fr)), all on the device: `_analyse_files` on the one file, as its own batch."""
    return file_features(_analyse_files(args, audio, sample_rate, slices, units_encoder, f0_extractor, key, units_batch_samples,
                                        solo=True), 0)


def _analyse_files(args, audios, sample_rate, slices, units_encoder, f0_extractor, keys, units_batch_samples, solo=False):
    """The one analysis body -> `analyse_many`'s dict.  `solo`: `audios`, `slices` and `keys` are those of ONE file (`_analyse`),
    which is a list of one file that is its own batch."""
    if solo:
        # A single file is its own batch: its row is the file itself, unpadded, and the analysers are called without counts -
        # their solo form: its bits, its draw of the dither seed, the volume of a fractional hop - as is the encoder for a slice
        # that is a group of its own; a given slice that reaches past the file's end is cut there, as a Python slice is.
        audios, slices = [audios.reshape(-1)], None if slices is None else [slices]
        who, batch_of_files, lone_slices = "convert", False, units_batch_samples is None
    else:
        who, batch_of_files, lone_slices = "analyse_many", True, False
    hop_size = int(args.data.block_size) * sample_rate / int(args.data.sampling_rate)
    if f0_extractor.sample_rate != sample_rate or f0_extractor.hop_size != hop_size:
        raise ValueError(f"{who}: the f0 extractor works at {f0_extractor.sample_rate} Hz with hop {f0_extractor.hop_size}; "
                         f"the audio is at {sample_rate} Hz with hop {hop_size}")
    F = len(audios)
    dev = next((a.device for a in audios if isinstance(a, torch.Tensor) and a.is_cuda), torch.device(f0_extractor.device))
    files = {"hop_size": hop_size, "sample_rate": sample_rate, "device": dev, "pieces": [], "units": [], "n_samples": [],
             "n_frames": []}
    if F == 0:
        return files
    keys = _per_file(keys, F, f"{who}: keys")
    if slices is not None and len(slices) != F:
        raise ValueError(f"{who}: slices of {len(slices)} files for {F} files")
    counts = [int(a.shape[0]) if getattr(a, "ndim", 0) == 1 else -1 for a in audios]
    if min(counts) < 1:
        raise ValueError(f"{who}: every file must be mono audio of shape (T,) with T >= 1")
    ctx = hipddsp.context_for(dev)
    # The width of a batch of files is the longest file's, rounded up to 4 samples: every file's row then starts on 16 bytes, and
    # with the slice starts of an integral hop (multiples of it) the gather of the encoder's rows takes its 16-byte loads.  Not
    # where the rounding would add a frame to the volume's width (the longest file within 3 samples of a hop multiple).
    width, ragged = max(counts), counts if batch_of_files else None
    if batch_of_files and -(-width // 4) * 4 // int(hop_size) == width // int(hop_size):
        width = -(-width // 4) * 4
    if not batch_of_files:                                      # the file is the row
        a = audios[0]
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) if isinstance(a, np.ndarray) else a
        x = a.to(dev, torch.float32).contiguous()[None]
    elif all(isinstance(a, np.ndarray) for a in audios):        # padded on the host: one upload
        host = np.zeros((F, width), dtype=np.float32)
        for k, a in enumerate(audios):
            host[k, :counts[k]] = a
        x = torch.from_numpy(host).to(dev)
    else:
        x = torch.zeros(F, width, device=dev)
        for k, a in enumerate(audios):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) if isinstance(a, np.ndarray) else a
            x[k, :counts[k]] = a.to(dev, torch.float32)
    if slices is None:                                                 # `split` of every row, in one call
        table, count, _ = Slicer(sr=sample_rate, threshold=SLICER_DB_THRESH, min_length=SLICER_MIN_LEN).chunks(x, n_samples=ragged)
        host = torch.cat([count, table.reshape(-1)]).cpu().numpy()     # the call's one read-back in front of the result
        ctx.poll_error()
        rows = host[F:].reshape(F, -1, 3)
        slices = [[(int(a), int(b)) for a, b, _ in rows[k, :host[k]] if a != b] for k in range(F)]
    n_frames = [int(n // hop_size) + 1 for n in counts]
    pieces = piece_table(slices, hop_size)
    if not batch_of_files:                                      # the cut at the file's end: `audio[start:end]` of main.py:41-46
        cut = [min(row[4], counts[0] - row[3]) for row in pieces]
        pieces = [(0, row[1], int(ns // hop_size) + 1, row[3], ns) for row, ns in zip(pieces, cut)]
    for k, start_frame, n, start_sample, n_samples in pieces:
        if start_sample < 0 or n_samples < 1 or start_sample + n_samples > counts[k] or start_frame + n > n_frames[k]:
            raise ValueError(f"{who}: file {k}: the slice at frame {start_frame} ({n} frames, samples {start_sample} to "
                             f"{start_sample + n_samples}) leaves the file's {counts[k]} samples / {n_frames[k]} frames")
    # Every upload of the call stands here, in front of its launches: a blocking copy behind them would hold the host until the
    # device has caught up, and the device would then wait while the host issues the encoder and the forwards.
    counts_dev = ctx.ragged_counts(counts + n_frames).reshape(2, F)
    files.update(audio=x, n_samples=counts, n_frames=n_frames, pieces=pieces, n_samples_dev=counts_dev[0],
                 n_frames_dev=counts_dev[1],
                 key_factor=torch.tensor([2 ** (float(key) / 12) for key in keys], dtype=torch.float32).to(dev))
    units = [None] * len(pieces)
    groups = group_pieces(pieces, 0 if units_batch_samples is None else int(units_batch_samples), by_samples=True)
    table, _, bounds = _upload_pieces(ctx, files, groups)
    files.update(f0=f0_extractor.extract(x, uv_interp=True, n_samples=ragged).contiguous(),
                 volume=ctx.volume_extract(x, hop_size, ragged))
    for group, (a, b) in zip(groups, bounds):
        n_rows = [pieces[i][4] for i in group]
        wav, _, _ = ctx.pieces_gather(table[a:b], files["n_samples_dev"], files["n_frames_dev"], audio=x, S_max=max(n_rows))
        got = units_encoder.encode(wav, sample_rate, hop_size, n_samples=None if lone_slices else n_rows)
        for j, i in enumerate(group):
            units[i] = got[j:j + 1, :pieces[i][2]].clone()
    files["units"] = units
    return files


def file_features(files, k):
    """File k of `analyse_many`'s result in `_analyse`'s form -> (segments [(start_frame, units (1, n, n_unit))], f0 (1, Fr, 1)
    shifted by the file's key, volume (1, Fr)): what `render_device` takes for that file alone."""
    n = files["n_frames"][k]
    segments = [(row[1], u) for row, u in zip(files["pieces"], files["units"]) if row[0] == k]
    f0 = files["f0"][k:k + 1, :n, None] * files["key_factor"][k]
    return segments, f0, files["volume"][k:k + 1, :n]


def file_of_features(segments, f0, volume):
    """The inverse of `file_features`: (segments, f0 (1, Fr, 1) already shifted, volume (1, Fr)) -> the dict of a list of one
    file, as `_render_files` takes it.  The key factor is 1.0 (an exact product); a piece row is (0, start frame, frames of
    units, 0, 0), the audio half unused.  n_frames is the volume's length (the gate's dilation ends where the given track
    ends) and f0 is cut or zero-padded to it: a segment inside both tracks, which `render_device` checks first, reads neither."""
    n = volume.shape[1]
    track = f0[0, :n, 0].float()
    if track.shape[0] < n:
        track = torch.nn.functional.pad(track, (0, n - track.shape[0]))
    counts = torch.tensor([[0], [n]], dtype=torch.int32).to(f0.device)          # (one upload)
    return {"device": f0.device, "n_samples": [0], "n_frames": [n], "n_samples_dev": counts[0], "n_frames_dev": counts[1],
            "f0": track[None].contiguous(), "volume": volume.float().contiguous(), "key_factor": torch.ones(1, device=f0.device),
            "pieces": [(0, int(start), units.size(1), 0, 0) for start, units in segments],
            "units": [units for _, units in segments]}


@torch.no_grad()
def render_many_device(model, args, files, spk_ids, spk_mix_rows=None, threshold_db=-60, enhancer=None, enhancer_adaptive_key=0,
                       noise_seed=None, batch_frames=None, noise=None, enhancer_batch_samples=None):
    """`render_device` for the files of `analyse_many` in one pass -> (fp64 device tensor holding every file, [(base, total)]
    per file, sample rate): file k is out[base:base + total], what `render_device` gives for it alone (`stitch_plan_many`
    states the layout; the gaps in front of odd bases are exact zeros, a file without slices has total 0).
    `group_segments` runs over the slices of ALL files (`batch_frames` padded frames per group; None: a slice per group), so
    short files share their forwards.  Per group: one `ddsp_pieces_gather` (the rows' f0 times their file's key factor, and
    volume), one ragged forward with every row's own speaker, one `ddsp_volume_gate_files`; then the enhancer in ragged groups
    over all pieces (`enhancer_batch_samples`; one `enhancer_adaptive_key` serves the call, as `enhance_batch` takes it) and ONE
    `ddsp_stitch`.
    spk_ids: one speaker id or one per file (ints or a tensor).  spk_mix_rows: (ids (F, K) int32, w (F, K) fp32) device
    tables, a speaker mix per FILE in place of `spk_ids`; every row takes its file's.
    noise: noise[k][i] is the (n * block,) U[0,1) draw of file k's slice i, as `render_device`'s `noise` is per segment.
    noise_seed: group g - the g-th group of `group_segments` over the pieces in `files['pieces']` order - draws with the seed
    (noise_seed + g * 2**32) mod 2**64, and the in-kernel draw is a hash of (seed, row, sample).  The grouping depends on the
    files' slice lengths and `batch_frames` alone, so the same call twice gives the same bits; two identical files in one call
    lie in different rows or different groups, so their noise differs.  (The draws are not those of `render_device` per file.)"""
    F, pieces, dev = len(files["n_frames"]), files["pieces"], files["device"]
    if F and noise is not None and ([len(x) for x in noise] != [sum(1 for row in pieces if row[0] == k) for k in range(F)]):
        raise ValueError("render_many_device: noise must hold one list per file with one draw per slice")

    def speaker(file_of_row, order):                      # every row takes its file's speaker, or its file's mix
        rows = file_of_row.long()
        if spk_mix_rows is None:
            spk = torch.tensor(_per_file(spk_ids, F, "render_many_device: spk_ids"), dtype=torch.int64).to(dev)
            spk, mix = spk.index_select(0, rows).reshape(-1, 1), None
        else:
            if spk_mix_rows[0].shape[0] != F or spk_mix_rows[1].shape[0] != F:
                raise ValueError(f"render_many_device: spk_mix_rows must hold one row per file ({F})")
            mix = [t.index_select(0, rows).contiguous() for t in spk_mix_rows]
            spk = torch.ones(len(pieces), 1, dtype=torch.int64, device=dev)      # (not read: the mix stands in its place)

        def of_group(a, b):
            return {"spk_id": spk[a:b]} if mix is None else {"spk_id": spk[a:b], "spk_mix_rows": (mix[0][a:b], mix[1][a:b])}
        return of_group

    def seed_of_group(g, starts):
        return (int(noise_seed) + (g << 32)) & ((1 << 64) - 1)
    return _render_files(model, args, files, speaker, None if noise_seed is None else seed_of_group,
                         None if noise is None else [x for per_file in noise for x in per_file], threshold_db=threshold_db,
                         enhancer=enhancer, enhancer_adaptive_key=enhancer_adaptive_key, batch_frames=batch_frames,
                         enhancer_batch_samples=enhancer_batch_samples)


@torch.no_grad()
def render_device(model, args, segments, f0, volume, spk_id, spk_mix_dict=None, threshold_db=-60, enhancer=None,
                  enhancer_adaptive_key=0, noise_seed=None, batch_frames=None, noise=None, enhancer_batch_samples=None):
    """`render` with its keywords, the result left on the device -> (fp64 device tensor (total,), sample rate), equal to
    `render`'s array: `_render_files` on `file_of_features(segments, f0, volume)`, a list of one file, under `render`'s rules - a
    group draws with the seed noise_seed + its smallest start frame, `spk_id` and `spk_mix_dict` go to the model untouched (one
    speaker for every row).  `batch_frames=None` / `enhancer_batch_samples=None`: one slice per group.  Nothing is read back
    between the first forward and the returned tensor beyond what `Enhancer.enhance_batch` itself reads."""
    for start, units in segments:
        n = units.size(1)
        if start < 0 or start + n > f0.shape[1] or start + n > volume.shape[1]:
            raise ValueError(f"render_device: the segment at frame {start} has {n} frames of units but f0 / volume cover "
                             f"{f0.shape[1]} / {volume.shape[1]} frames of the file")
    return _render_file(model, args, file_of_features(segments, f0, volume), spk_id, spk_mix_dict, noise_seed, noise,
                        threshold_db=threshold_db, enhancer=enhancer, enhancer_adaptive_key=enhancer_adaptive_key,
                        batch_frames=batch_frames, enhancer_batch_samples=enhancer_batch_samples)


def _render_file(model, args, files, spk_id, spk_mix_dict, noise_seed, noise, **stages):
    """`_render_files` (`stages`: its keywords) on a list of one file under `render`'s seed and speaker rules -> (out, rate)."""
    def speaker(file_of_row, order):
        return lambda a, b: {"spk_id": spk_id, "spk_mix_dict": spk_mix_dict}

    def seed_of_group(g, starts):
        return noise_seed + min(starts)
    out, _, sr_o = _render_files(model, args, files, speaker, None if noise_seed is None else seed_of_group, noise, **stages)
    return out, sr_o


def _render_files(model, args, files, speaker, seed_of_group, noise, *, threshold_db, enhancer, enhancer_adaptive_key,
                  batch_frames, enhancer_batch_samples, jobs=None):
    """The one render body, as `render_many_device` states it.  What its callers differ in is passed in.  speaker: called once
    with the file of every row (int32 device, rows in the groups' order) and the rows' indices in that order -> a function of a
    group's row range (a, b) giving the model's speaker keywords.  seed_of_group: None (the model draws its seed) or a function
    of the group's number and its rows' start frames -> the group's noise seed.  noise: None or one draw per row, in row order.
    jobs: None - a row is a piece of `files`, an output is a file, `model` renders every group - or (models, `job_table`'s dict
    with its key factors uploaded as 'key_factor_dev'): a row is a piece of a job's file (six columns: `ddsp_pieces_gather_jobs`
    reads the file's features in place and takes the JOB's key factor), an output is a job, the groups are `job_groups`' and
    each is rendered by its model.  The gate takes a row's file either way."""
    block, sr, dev = int(args.data.block_size), int(args.data.sampling_rate), files["device"]
    F, pieces, units = len(files["n_frames"]), files["pieces"], files["units"]
    if F == 0 or (jobs is not None and not jobs[1]["model_of_job"]):
        return torch.zeros(0, dtype=torch.float64, device=dev), [], sr
    ctx = hipddsp.context_for(dev)
    for k, start, n, _, _ in pieces:
        if start < 0 or start + n > files["n_frames"][k]:
            raise ValueError(f"offline render: file {k}: the segment at frame {start} has {n} frames of units but f0 / volume "
                             f"cover {files['n_frames'][k]} frames of the file")
    budget = 0 if batch_frames is None else int(batch_frames)
    if jobs is None:
        rows, unit_of, owner, n_out, key = pieces, range(len(pieces)), 0, F, {"key_factor": files["key_factor"]}
        groups = group_pieces(pieces, budget)
        model_of_group = [model] * len(groups)
    else:
        models, table = jobs
        rows, unit_of, owner, n_out = table["rows"], table["piece_of_row"], 5, len(table["model_of_job"])
        key = {"key_timeline": table["key_tables_dev"]} if "key_tables_dev" in table else {"key_factor": table["key_factor_dev"]}
        numbered = job_groups(table, len(models), budget)
        groups, model_of_group = [group for _, group in numbered], [models[m] for m, _ in numbered]
        table_models = [m for m, _ in numbered]
    given = None if jobs is None else rows
    formant = None if jobs is None else jobs[1].get("formant")       # (models with a formant among their jobs, tables, f0 of ones)
    tune = None if jobs is None else jobs[1].get("tune")             # (the settings of all jobs, when one of them has a tune)
    retrieve = None if jobs is None else jobs[1].get("retrieve")     # (bank, index and ratio of all jobs, k: when one names an index)
    table, cols, bounds = _upload_pieces(ctx, files, groups, given)
    speaker_of_rows = speaker(cols[0], [i for group in groups for i in group])
    out = [None] * len(rows)
    for g, (group, (a, b)) in enumerate(zip(groups, bounds)):
        counts = [rows[i][2] for i in group]
        u, _ = stack_rows([units[unit_of[i]][0] for i in group])
        if retrieve is not None:                                     # behind the encoder: the group's stacked units, in place
            bank, index_of_job, ratio_of_job, k = retrieve
            job_of_row = cols[5, a:b].long()
            bank.reserve(u.shape[0], u.shape[1], k)
            ctx.units_retrieve_(u, bank, index_of_job[job_of_row], ratio_of_job[job_of_row], k=k, n_frames=cols[2, a:b].contiguous())
        _, f, v = ctx.pieces_gather(table[a:b], files["n_samples_dev"], files["n_frames_dev"], f0=files["f0"],
                                    volume=files["volume"], N_max=max(counts), **key)
        if tune is not None:                                         # behind the key: the output lands in the scale
            ctx.f0_tune_(f, *tune, n_frames=cols[2, a:b], owner=cols[5, a:b])
        kw = {} if seed_of_group is None else {"noise_seed": seed_of_group(g, [rows[i][1] for i in group])}
        if noise is not None:
            kw["noise"] = stack_rows([noise[i].reshape(-1) for i in group])[0]
        if formant is not None and table_models[g] in formant[0]:
            # the rows' factors per frame: the key timeline rule on an f0 of ones, one launch (0 past a row's count, where the
            # warp reads no factor)
            _, fac, _ = ctx.pieces_gather(table[a:b], files["n_samples_dev"], files["n_frames_dev"], f0=formant[2],
                                          N_max=max(counts), key_timeline=formant[1])
            signal = model_of_group[g].forward_formant(u, f[:, :, None], v, formant=fac, n_frames=counts, **speaker_of_rows(a, b),
                                                       **kw)[0].contiguous()
        else:
            signal = model_of_group[g](u, f[:, :, None], v, n_frames=counts, **speaker_of_rows(a, b), **kw)[0].contiguous()
        ctx.volume_gate_rows_(signal, files["volume"], cols[1, a:b], cols[2, a:b], threshold_db, block,
                              file_dev=cols[0, a:b], file_frames_dev=files["n_frames_dev"])
        for j, i in enumerate(group):
            out[i] = signal[j:j + 1, :counts[j] * block]
    sr_o = sr
    if enhancer is not None and rows:
        out, sr_o = _enhance_many(ctx, enhancer, out, files, sr, block, enhancer_adaptive_key,
                                  0 if enhancer_batch_samples is None else enhancer_batch_samples, given, key, tune)
    per_out = [[i for i, row in enumerate(rows) if row[owner] == k] for k in range(n_out)]
    spans, p, fade, total = stitch_plan_many([[rows[i][1] for i in idx] for idx in per_out],
                                             [[out[i].shape[-1] for i in idx] for idx in per_out], block, sr, sr_o)
    return ctx.stitch(out, p, fade, total), spans, sr_o


def _enhance_many(ctx, enhancer, gated, files, sr, block, adaptive_key, enhancer_batch_samples, rows=None, key=None, tune=None):
    """The device path's enhancer loop over the gated pieces of all files: one `Enhancer.enhance_batch` per group of
    `group_segments` over the sample lengths, every row with its own file's shifted f0 (one `ddsp_pieces_gather` per group).
    rows, key: `job_table`'s rows and the jobs' keys - `pieces_gather`'s keyword `key_factor` or `key_timeline` with its value -
    in place of the files' (one enhancer serves all models).  tune: the jobs' pitch-correction settings (`tune_tables` on the
    device) or None: every row's f0 is corrected as the render corrected it - the same kernel on the same row."""
    pieces = files["pieces"] if rows is None else rows
    key = {"key_factor": files["key_factor"]} if key is None else key
    groups = group_segments([g.shape[-1] for g in gated], int(enhancer_batch_samples))
    table, cols, bounds = _upload_pieces(ctx, files, groups, rows)
    out, sr_o = [None] * len(gated), sr
    for group, (a, b) in zip(groups, bounds):
        wav, counts = stack_rows([gated[i][0] for i in group])
        n_f0 = [pieces[i][2] for i in group]
        _, tracks, _ = ctx.pieces_gather(table[a:b], files["n_samples_dev"], files["n_frames_dev"], f0=files["f0"],
                                         N_max=max(n_f0), **key)
        if tune is not None:
            ctx.f0_tune_(tracks, *tune, n_frames=cols[2, a:b], owner=cols[5, a:b])
        got, sr_o, n_out = enhancer.enhance_batch(wav, sr, tracks[:, :, None], block, counts, adaptive_key=adaptive_key, n_f0=n_f0)
        for j, i in enumerate(group):
            out[i] = got[j:j + 1, :n_out[j]]
    return out, sr_o


def _models_of(who, model, models):
    """`models=` and the positional model -> the list of models (`StreamBank`'s rule: with `models`, `model` is None or
    models[0] itself; without, the list of that one model)."""
    if models is None:
        return [model]
    if not (isinstance(models, (tuple, list)) and len(models)):
        raise ValueError(f"{who}: models must be a non-empty list of synthesisers")
    if model is not None and model is not models[0]:
        raise ValueError(f"{who}: with models= the positional model is None or models[0] itself (it names model 0)")
    return list(models)


@torch.no_grad()
def render_jobs_device(models, args, files, jobs, threshold_db=-60, enhancer=None, enhancer_adaptive_key=0, noise_seed=None,
                       batch_frames=None, noise=None, enhancer_batch_samples=None, key_tables_always=False, indices=None,
                       retrieve_k=8):
    """`render_many_device` for JOBS over the files of ONE `analyse_many` (analysed with keys=0: the key is the job's) -> (fp64
    device tensor holding every job, [(base, total)] per job in job order, sample rate).  jobs: a sequence of (file,
    model_index, spk, key) into `files` and `models`, or of `Job` records, which name the entries below (`job_table` states and
    checks them: ValueError before any launch; the list is read through `Job.of` once, here).  Job j
    is out[base:base + total], what `render_many_device` gives for that file alone with that model, speaker and key.
    The groups are formed per model over the slices of that model's jobs (`job_groups`), each one ragged forward of its model:
    a row reads its file's f0 and volume in place through the six-column table (`ddsp_pieces_gather_jobs`) - f0 times its
    JOB's key factor - takes its job's speaker, and is gated by its FILE's volume.  The units of a file's slices serve every
    job over it.  A model whose jobs all name a plain id gets `spk_id` rows; one with a mix among its jobs gets `spk_mix_rows`
    for all of them (a plain id is the row {id: 1.0}); one with a `SpeakerTimeline` among its jobs renders ALL its groups with
    a mix per frame - one `ddsp_mix_timeline` launch per group turns the jobs' breakpoints (file time) into the weights of the
    group's rows, wherever in their files the rows lie, and its id and dict jobs are timelines of one breakpoint.  The enhancer - one for all models, one `enhancer_adaptive_key` per
    call - takes ragged groups over the rows of all jobs, and ONE `ddsp_stitch` places every job (`stitch_plan_many` over jobs:
    even bases, no fade across jobs).
    A job's key may be a `KeyTimeline`, a key that moves over the file.  Without one among the jobs the call is the call above,
    bit for bit.  With one, EVERY gather of the call - the render groups and the enhancer's f0 - goes through
    `ddsp_pieces_gather_keys` with the `key_tables` of all jobs, uploaded once: a row's f0 is its file's times the factor at
    every frame's own file frame, a numeric key is the one breakpoint at frame 0 and keeps its bits, and the enhancer
    (`enhancer_adaptive_key='auto'` too) sees the same moving f0.  key_tables_always: take that path whatever the keys are.
    A job may be a 5-tuple (file, model_index, spk, key, formant): a FORMANT shift in semitones, a number or a
    `FormantTimeline`.  A model with a formant among its jobs renders all its groups through `forward_formant` with a factor per
    frame - the key timeline rule at every frame's own file frame, one `ddsp_pieces_gather_keys` launch per group over an f0 of
    ones -; a model without one takes the path above, bit for bit.  The enhancer is not told of the shift: it follows f0.
    A job may be a 6-tuple (file, model_index, spk, key, formant, tune): PITCH CORRECTION, a `PitchTune` or None (the formant may
    be None as well).  With a tune among the jobs the settings of all jobs go up once (`tune_tables`) and every gather of f0 -
    the render groups and the enhancer's - is followed by one `ddsp_f0_tune` launch on the group's rows, behind the key, with
    the rows' jobs as their owners: the rows of a job without a tune keep their bits, and the enhancer sees the corrected f0.
    The correction restarts at every slice.  Without a tune among the jobs nothing is launched: the call above, bit for bit.
    A job may be a 7-tuple (file, model_index, spk, key, formant, tune, index): UNIT RETRIEVAL, (index_number, ratio) into
    `indices` (a `UnitIndexBank` on the files' device) or None.  With an index among the jobs the rows' settings go up once
    (`index_tables`) and every render group's stacked units pass through one `Context.units_retrieve_` (k = `retrieve_k`) with
    the group's frame counts, right where the encoder's units enter the synthesiser: the rows of a job without an index keep
    their bits.  Without an index among the jobs nothing is launched: the call above, bit for bit.  ValueError for an index
    among the jobs without `indices`, an index number outside the bank, or a bank whose width is not the units'.
    A job may be an 8-tuple (file, model_index, spk, key, formant, tune, index, envelope): the ENVELOPE MIX, an `EnvelopeMix`
    (a job without one is the shorter tuple; RVC's `rms_mix_rate`; include/ddsp_amd.h states the rule).  With an envelope among
    the jobs three launches follow the stitch: the frame RMS of the files' audio, the frame RMS of the job spans of the stitched tensor - at the OUTPUT's rate,
    the enhancer's when there is one - and the apply, in place, every job with its own rate and its file as the source.  The
    span of a job without an envelope keeps its bits, the spans themselves do not move, and `to_pcm16` sees the matched
    output.  Without an envelope among the jobs nothing is launched: the call above, bit for bit.
    noise: noise[j][i] is the draw of job j's slice i.  noise_seed: group g of `job_groups` - numbered model by model, in
    `models` order - draws with (noise_seed + g * 2**32) mod 2**64."""
    models = _models_of("render_jobs_device", None, models)
    dev, pieces, n_files = files["device"], files["pieces"], len(files["n_frames"])
    if indices is not None and not isinstance(indices, UnitIndexBank):
        raise ValueError(f"render_jobs_device: indices must be a UnitIndexBank, got {type(indices).__name__}")
    jobs = [Job.of(j, job) for j, job in enumerate(jobs)]
    table = job_table(pieces, n_files, jobs, models, None if indices is None else len(indices))
    J = len(table["model_of_job"])
    rate = (_model_field(models[0], "sampling_rate"), _model_field(models[0], "block_size"))       # (the models agree in it)

    def given(values):                   # a control as every job carries it, or None when no job does: nothing goes up for it
        return values if any(v is not None for v in values) else None

    def upload(tables):
        return tuple(t.to(dev) for t in tables)
    settings, formants, envelopes, tunes = (given(of(jobs)) for of in (job_indices, job_formants, job_envelopes, job_tunes))
    if settings:
        if indices is None:
            raise ValueError("render_jobs_device: a job names an index, but the call has no indices=")
        if files["units"] and (indices.device != files["units"][0].device or indices.channels != int(files["units"][0].shape[-1])):
            raise ValueError(f"render_jobs_device: the bank holds {indices.channels} channels on {indices.device}, the files' units "
                             f"are on {dev}")
        if isinstance(retrieve_k, bool) or not isinstance(retrieve_k, int) or not 1 <= retrieve_k <= hipddsp.MAX_RETRIEVE_K:
            raise ValueError(f"render_jobs_device: retrieve_k must be an int in 1..{hipddsp.MAX_RETRIEVE_K}, got {retrieve_k!r}")
        table["retrieve"] = (indices, *upload(index_tables(settings)), retrieve_k)
    if J and noise is not None and [len(x) for x in noise] != [len(s) for s in table["starts_per_job"]]:
        raise ValueError("render_jobs_device: noise must hold one list per job with one draw per slice of its file")
    if J and (key_tables_always or any(isinstance(k, KeyTimeline) for k in table["keys"])):
        # a key that moves: the breakpoint tables of ALL jobs go up once and serve every gather of the call
        table["key_tables_dev"] = upload(key_tables(table["keys"], *rate))
    elif J:
        table["key_factor_dev"] = torch.tensor(table["key_factor"], dtype=torch.float32).to(dev)
    if formants:
        # a formant among the jobs: its model renders ALL its groups through `forward_formant`; the breakpoint tables of all jobs
        # (a job without a shift: 0 semitones, factor 1) go up once, with an f0 of ones that `ddsp_pieces_gather_keys` turns into
        # every group's factor rows
        table["formant"] = ({table["model_of_job"][j] for j, f in enumerate(formants) if f is not None},
                            upload(formant_tables(formants, *rate)), torch.ones_like(files["f0"]))
    envelope = None
    if envelopes:
        if "audio" not in files:
            raise ValueError("render_jobs_device: an envelope among the jobs needs the files' audio (`analyse_many`'s dict)")
        mix_rate, hop_seconds, frames = envelope_tables(envelopes)
        EnvelopeMix(1.0, hop_seconds, frames).setting(files["sample_rate"])      # (a hop below one sample: refused here)
        envelope = (mix_rate.to(dev), hop_seconds, frames)
    if tunes:
        table["tune"] = upload(tune_tables(tunes, *rate))

    def speaker(file_of_row, order):
        # Every row takes its job's speaker, from host tables uploaded once in front of the launches (the job of a row is known
        # here: nothing indexes with a device column).  The rows of a model are contiguous: the groups are numbered model by model.
        jobs_in_order = [table["rows"][i][5] for i in order]
        ctx = hipddsp.context_for(dev)
        spk = torch.tensor([s if isinstance(s, int) else 1 for s in (table["speakers"][j] for j in jobs_in_order)],
                           dtype=torch.int64).reshape(-1, 1).to(dev)
        mixes, timelines = {}, {}
        for m, model in enumerate(models):
            mine = [a for a, j in enumerate(jobs_in_order) if table["model_of_job"][j] == m]
            of_rows = [table["speakers"][jobs_in_order[a]] for a in mine]
            if any(isinstance(s, SpeakerTimeline) for s in of_rows):
                # a model with a timeline among its jobs: the per-frame mix for ALL its groups, its id and dict jobs as constant
                # timelines; the tables go up once, every group's weights come from one `ddsp_mix_timeline` launch
                jobs_of_m = [j for j, mj in enumerate(table["model_of_job"]) if mj == m]
                timelines[m] = [t.to(dev) for t in timeline_tables(table["speakers"], jobs_of_m, model._sr, model._hop)]
            elif any(isinstance(s, dict) for s in of_rows):
                ids, w = hipddsp.mix_rows(of_rows, max(len(s) if isinstance(s, dict) else 1 for s in of_rows),
                                          int(model.unit2ctrl.n_spk))
                mixes[m] = (mine[0], ids.to(dev), w.to(dev))

        def of_group(a, b):
            m = table["model_of_job"][jobs_in_order[a]]
            if m in timelines:
                N_max = max(table["rows"][i][2] for i in order[a:b])
                return {"spk_id": spk[a:b], "spk_mix_rows": ctx.mix_timeline(files["table"][a:b], *timelines[m], N_max)}
            if m not in mixes:
                return {"spk_id": spk[a:b]}
            first, ids, w = mixes[m]
            return {"spk_id": spk[a:b], "spk_mix_rows": (ids[a - first:b - first], w[a - first:b - first])}
        return of_group

    def seed_of_group(g, starts):
        return (int(noise_seed) + (g << 32)) & ((1 << 64) - 1)
    result, spans, sr_o = _render_files(None, args, files, speaker, None if noise_seed is None else seed_of_group,
                                        None if noise is None else [x for per_job in noise for x in per_job],
                                        threshold_db=threshold_db, enhancer=enhancer, enhancer_adaptive_key=enhancer_adaptive_key,
                                        batch_frames=batch_frames, enhancer_batch_samples=enhancer_batch_samples,
                                        jobs=(models, table))
    if envelope is not None:
        _envelope_mix_jobs(files, jobs, envelope, result, spans, sr_o)
    return result, spans, sr_o


def _envelope_mix_jobs(files, jobs, envelope, result, spans, sr_o):
    """The envelope mix of a jobs call, in place on the stitched tensor: three launches behind the stitch.  One
    `Context.envelope_rms` over the files' audio at the files' sample rate, one over the job spans of `result` at `sr_o` (the
    enhancer's rate when there is one: the hop is taken from it), one `Context.envelope_mix_` with every job as the owner of
    its span and the job's file as its source.  envelope: (`envelope_tables`' rates on the device, hop_seconds, frames)."""
    rate, hop_seconds, frames = envelope
    named = [j for j, (_, total) in enumerate(spans) if total >= 1]          # (a job over a file without a slice has no samples)
    if not named:
        return
    dev = files["device"]
    ctx = hipddsp.context_for(dev)
    one = EnvelopeMix(1.0, hop_seconds, frames)
    hop_in, hop_out = one.setting(files["sample_rate"]), one.setting(sr_o)
    n_max = max(spans[j][1] for j in named)
    table = torch.tensor([[spans[j][0], spans[j][1], j, jobs[j].file] for j in named], dtype=torch.int64).to(dev)   # one upload
    rows, owner, source = table[:, :2].contiguous(), table[:, 2].int(), table[:, 3].int()
    src = ctx.envelope_rms(files["audio"], hop_in, frames, n_samples=files["n_samples_dev"])
    env = ctx.envelope_rms(result, hop_out, frames, spans=rows, n_max=n_max)
    ctx.envelope_mix_(result, src, rate, env, hop_out, hop_in, files["n_samples_dev"], spans=rows, n_max=n_max, src_of_row=source,
                      owner=owner)


@torch.no_grad()
def convert_many_device(model, args, audios, sample_rate, units_encoder, f0_extractor, spk_ids=None, slices=None, keys=0,
                        batch_frames=None, spk_mix_rows=None, threshold_db=-60, enhancer=None, enhancer_adaptive_key=0,
                        noise_seed=None, enhancer_batch_samples=None, units_batch_samples=None, jobs=None, models=None,
                        noise=None, indices=None, retrieve_k=8):
    """`analyse_many` then `render_many_device`: a list of files from raw audio to one fp64 device tensor -> (out, [(base,
    total)] per file, sample rate).  Files are batched within ONE call's sample rate and enhancer key.
    jobs: None - one model (`model`), one speaker (`spk_ids`, required then) and one key per file, as above - or a sequence of
    (file, model_index, spk, key) or of `Job` records: every file is analysed ONCE, whatever the number of jobs over it, and rendered once per job
    (`render_jobs_device`) -> one span per job, in job order.  models: the synthesisers the jobs index (None: [model]; with it,
    `model` is None or models[0]).  With `jobs`, the speaker and the key are the job's: `spk_ids`, `spk_mix_rows` and `keys`
    must be left at their defaults (ValueError), and all tables are checked before anything is analysed (`job_table`).  An
    empty list of jobs gives an empty tensor and no spans, and analyses nothing.
    noise: `render_many_device`'s (per file) or `render_jobs_device`'s (per job) injected draws.
    indices, retrieve_k: `render_jobs_device`'s bank of unit indices for jobs with a seventh entry; they go with jobs=."""
    if jobs is None:
        if indices is not None:
            raise ValueError("convert_many_device: indices= goes with jobs= (a job's seventh entry names its index)")
        if models is not None:
            raise ValueError("convert_many_device: models= goes with jobs=; without jobs the one model is the positional one")
        if spk_ids is None and spk_mix_rows is None:
            raise ValueError("convert_many_device: spk_ids (or spk_mix_rows) is required without jobs=")
        check_units_width("convert_many_device", units_encoder, model)
        files = analyse_many(args, audios, sample_rate, slices, units_encoder, f0_extractor, keys, units_batch_samples)
        return render_many_device(model, args, files, spk_ids, spk_mix_rows=spk_mix_rows, threshold_db=threshold_db,
                                  enhancer=enhancer, enhancer_adaptive_key=enhancer_adaptive_key, noise_seed=noise_seed,
                                  batch_frames=batch_frames, noise=noise, enhancer_batch_samples=enhancer_batch_samples)
    if spk_ids is not None or spk_mix_rows is not None or not (isinstance(keys, numbers.Real) and keys == 0):
        raise ValueError("convert_many_device: with jobs= the speaker and the key are each job's: leave spk_ids, spk_mix_rows and "
                         "keys at their defaults")
    models = _models_of("convert_many_device", model, models)
    if indices is not None and not isinstance(indices, UnitIndexBank):
        raise ValueError(f"convert_many_device: indices must be a UnitIndexBank, got {type(indices).__name__}")
    jobs = [Job.of(j, job) for j, job in enumerate(jobs)]
    # every refusal of the tables, before anything is analysed
    job_table([], len(audios), jobs, models, None if indices is None else len(indices))
    if indices is None and any(s is not None for s in job_indices(jobs)):
        raise ValueError("convert_many_device: a job names an index, but the call has no indices=")
    check_units_width("convert_many_device", units_encoder, *models)
    if not jobs:
        return torch.zeros(0, dtype=torch.float64, device=next(models[0].parameters()).device), [], int(args.data.sampling_rate)
    files = analyse_many(args, audios, sample_rate, slices, units_encoder, f0_extractor, 0, units_batch_samples)
    return render_jobs_device(models, args, files, jobs, threshold_db=threshold_db, enhancer=enhancer,
                              enhancer_adaptive_key=enhancer_adaptive_key, noise_seed=noise_seed, batch_frames=batch_frames,
                              noise=noise, enhancer_batch_samples=enhancer_batch_samples, indices=indices, retrieve_k=retrieve_k)


@torch.no_grad()
def convert_device(model, args, audio, sample_rate, slices, units_encoder, f0_extractor, spk_id, batch_frames=None, key=0,
                   spk_mix_dict=None, threshold_db=-60, enhancer=None, enhancer_adaptive_key=0, noise_seed=None,
                   enhancer_batch_samples=None, units_batch_samples=None):
    """`convert_batched` ending as `render_device` does: `_analyse`'s analysis, its dict handed on as it is, then ragged
    rendering, one gate launch per group, the ragged enhancer and one stitch launch -> (fp64 device tensor (total,), sample
    rate), equal to `convert_batched`'s array.  One `.cpu()` of the result is the file's only read-back behind the slicer's."""
    check_units_width("convert_device", units_encoder, model)
    files = _analyse_files(args, audio, sample_rate, slices, units_encoder, f0_extractor, key, units_batch_samples, solo=True)
    return _render_file(model, args, files, spk_id, spk_mix_dict, noise_seed, None, threshold_db=threshold_db, enhancer=enhancer,
                        enhancer_adaptive_key=enhancer_adaptive_key, batch_frames=batch_frames,
                        enhancer_batch_samples=enhancer_batch_samples)


def convert_many(model, args, audios, sample_rate, units_encoder, f0_extractor, spk_ids=None, **kw):
    """`convert_many_device` (its keywords, `jobs=` and `models=` among them) with ONE `.cpu()` of the whole result, split into
    the files - the jobs, with `jobs=` - -> ([float64 numpy waveform per file or job], sample rate).  An empty list of files
    gives an empty list and launches nothing."""
    out, spans, sr_o = convert_many_device(model, args, audios, sample_rate, units_encoder, f0_extractor, spk_ids, **kw)
    host = out.cpu().numpy() if spans else np.zeros(0)
    return [host[base:base + total].copy() for base, total in spans], sr_o


def to_pcm16(result, spans):
    """The fp64 device tensor and spans of `convert_many_device` / `render_many_device` (or (0, n) of a single file's tensor)
    -> (int16 device tensor of the same layout, peak (len(spans),) fp64, clipped (len(spans),) int64, both on the device): one
    `ddsp_pcm16` launch, `main.pcm16` of every span bit for bit, zeros in the gaps, the largest |x| and the number of clipped
    samples of every span.  Reading the int16 tensor back moves 2 bytes per sample, not 8."""
    if not result.is_cuda:
        raise ValueError("to_pcm16: the result must be a device tensor (`main.pcm16` is the host statement)")
    return hipddsp.context_for(result.device).pcm16(result, spans)
