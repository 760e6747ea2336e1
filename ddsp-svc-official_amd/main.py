"""The reference's offline command line (`main.py`) over `infer_offline.convert_device`: a file goes from raw audio to the
stitched waveform on the device and is read back once.

    python main.py -m <model.pt> -i <in.wav> -o <out.wav> [-id 1] [-mix None] [-k 0] [-e true] [-pe crepe] [-fmin 50]
                   [-fmax 1100] [-th -60] [-eak 0] [-sr 44100]
    python main.py -m <model.pt> -i <folder of .wav> -o <output folder> ...     (every file in one `convert_many_device`)
    python main.py -m <model.pt> -i <folder> -o <folder> --jobs <jobs.yaml> ... (every file to every voice of the list)

`--jobs` names a YAML list of entries {model: <model.pt, default -m>, id: <speaker id, default 1> | mix: {id: weight} |
timeline: [{at: <seconds>, id: n} | {at: <seconds>, mix: {id: weight}}, ...] (a voice that glides over the file,
`infer_offline.SpeakerTimeline`), key: <semitones, default 0> | key_timeline: [{at: <seconds>, key: <semitones>}, ...] (a key
that moves over the file, `infer_offline.KeyTimeline`), formant: <semitones, default 0> | formant_timeline: [{at: <seconds>,
formant: <semitones>}, ...] (a formant shift, `infer_offline.FormantTimeline`), tune: {scale: "A minor" | notes: [<pitch class or
name>, ...], strength: <0..1, default 1>, retune_ms: <default 50>, a4: <Hz, default 440>} (pitch correction,
`infer_offline.PitchTune`), suffix: <text>}.  Every entry is applied to every `.wav` of the folder: file `name.wav` and suffix `s`
give `name_s.wav`.  All of it is ONE `convert_many_device(jobs=...)` - every file analysed once - and one read-back; `-id`,
`-mix` and `-k` are then unused.

`--formant_shift_key S` (long option only, default 0) shifts the formants of the file or folder by S semitones at the same pitch
(`forward_formant`); it runs through the jobs path, one job per file, and with `--jobs` it is the shift of the entries that
name none.

`--tune_scale "A minor"` (long options only; with `--tune_strength`, `--tune_retune_ms` and `--tune_a4`, defaults 1, 50 and 440)
pulls the sung f0 toward the notes of that scale (`infer_offline.PitchTune`, behind the key shift); it runs through the jobs
path like `--formant_shift_key`, and with `--jobs` it is the tune of the entries that name none.
`--index <file>` (an `infer_offline.UnitIndex.save` file; with `--index_ratio R`, default 0.5) blends every frame's units with
their nearest stored units of that voice (`ddsp_units_retrieve`); it runs through the jobs path too, and with `--jobs` it is the
index of the entries that name none - an entry names its own with `index: <file>` and `index_ratio: <0..1>`.
`--rms_mix_rate R` (0..1, RVC's option of that name) holds the output to the source's loudness envelope: R is the share of the
output's own envelope that is kept, 1 changes nothing (`infer_offline.EnvelopeMix`, RVC's `change_rms` behind the stitch).  It
runs through the jobs path too, and with `--jobs` it is the envelope of the entries that name none - an entry names its own
with `envelope: <rate>` or `envelope: {rate: <0..1>, hop_ms: <default 500>, frames: <2, 4, 6 or 8, default 2>}`; the entries of
one run share hop_ms and frames.

The options and their defaults are the reference's (`main.py:19-31`).  What differs, and why:
  * the key shift is applied once (the reference applies it twice);
  * `-pe` takes 'crepe' and 'ac' (`F0_Extractor`); 'parselmouth', 'dio' and 'harvest' raise as `F0_Extractor` does;
  * the input is read with `preprocess.load_wav` and, at another rate than `-sr`, resampled on the device with
    `resample.Resample` as `preprocess` does (the reference's librosa resamples with its own filter);
  * the output is 16-bit PCM through `scipy.io.wavfile.write` - what the reference's `sf.write` makes of a `.wav` by default;
    it is quantised on the device (`infer_offline.to_pcm16`; `pcm16` below is the host statement of the same numbers), so the
    read-back is the int16 samples, and an output with clipped samples is reported in one line;
  * the reference's md5-keyed f0 cache is left out: the f0 of a file takes milliseconds on the device.
"""
import argparse
import dataclasses
import os
from ast import literal_eval

import numpy as np
import torch

from controls import (EnvelopeMix, FormantTimeline, Job, KeyTimeline, PitchTune, SpeakerTimeline, UnitIndex, UnitIndexBank,
                      check_job_index)

# option, long name, type, default, help - the reference's table
_OPTIONS = (
    ("-m", "--model_path", str, None, "path to the model file"),
    ("-i", "--input", str, None, "path to the input audio file"),
    ("-o", "--output", str, None, "path to the output audio file"),
    ("-id", "--spk_id", str, 1, "speaker id (for multi-speaker model) | default: 1"),
    ("-mix", "--spk_mix_dict", str, "None", "mix-speaker dictionary (for multi-speaker model) | default: None"),
    ("-k", "--key", str, 0, "key changed (number of semitones) | default: 0"),
    ("-e", "--enhance", str, "true", "true or false | default: true"),
    ("-pe", "--pitch_extractor", str, "crepe", "pitch extractor type: crepe (default), ac"),
    ("-fmin", "--f0_min", str, 50, "min f0 (Hz) | default: 50"),
    ("-fmax", "--f0_max", str, 1100, "max f0 (Hz) | default: 1100"),
    ("-th", "--threhold", str, -60, "response threhold (dB) | default: -60"),
    ("-eak", "--enhancer_adaptive_key", str, 0, "adapt the enhancer to a higher vocal range (number of semitones) | default: 0"),
    ("-sr", "--sampling_rate", int, 44100, "Audio sampling rate"),
)


def parse_args(args=None, namespace=None):
    """The reference's options with its defaults; `-m`, `-i` and `-o` are required."""
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    for short, long, kind, default, text in _OPTIONS:
        parser.add_argument(short, long, type=kind, required=default is None, default=default, help=text)
    # (absent from the namespace unless given: the reference's options are the namespace of a plain call)
    parser.add_argument("--formant_shift_key", type=str, default=argparse.SUPPRESS, help="formant shift (number of semitones, "
                        "positive: brighter) for the file or folder | default: 0")
    parser.add_argument("--tune_scale", type=str, default=argparse.SUPPRESS, help="pitch correction toward the notes of a scale, "
                        "'<tonic> [major | minor | chromatic | major_pentatonic | minor_pentatonic]' such as 'A minor' | default: off")
    parser.add_argument("--tune_strength", type=str, default=argparse.SUPPRESS, help="share of the correction applied, 0..1 | default: 1")
    parser.add_argument("--tune_retune_ms", type=str, default=argparse.SUPPRESS, help="retune time in milliseconds, 0: at once | default: 50")
    parser.add_argument("--tune_a4", type=str, default=argparse.SUPPRESS, help="the Hz of A4 | default: 440")
    parser.add_argument("--index", type=str, default=argparse.SUPPRESS, help="unit retrieval: a UnitIndex file of the target voice")
    parser.add_argument("--index_ratio", type=str, default=argparse.SUPPRESS, help="share of the retrieved units, 0..1 | default: 0.5")
    parser.add_argument("--rms_mix_rate", type=str, default=argparse.SUPPRESS, help="envelope mix: the share of the output's own "
                        "loudness envelope that is kept, 0..1; 0 gives it the source's | default: off (1)")
    parser.add_argument("--jobs", type=str, default=argparse.SUPPRESS, help="YAML list of {model, id | mix, key, suffix}: every entry is applied "
                        "to every .wav of the input folder")
    return parser.parse_args(args=args, namespace=namespace)


def pcm16(wave):
    """float waveform -> int16 as libsndfile writes a 16-bit file from floats: scaled by 2^15, rounded to nearest, clipped."""
    return np.clip(np.rint(np.asarray(wave, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def _write_pcm(result, spans, paths, sr_o):
    """The waveforms out[base:base + total] of `spans` as 16-bit files at `paths`: quantised on the device, ONE read-back of the
    int16 tensor with the spans' peak and clipped counts behind it, a warning line per output that clipped."""
    from scipy.io import wavfile

    from infer_offline import to_pcm16
    pcm, peak, clipped = to_pcm16(result, spans)
    tail = torch.cat([peak.view(torch.int16), clipped.view(torch.int16)])
    host = torch.cat([pcm, tail]).cpu().numpy()                    # the one read-back
    stats = host[pcm.numel():].copy()                              # (aligned for the 8-byte views, whatever the length)
    peak, clipped = stats[:4 * len(spans)].view(np.float64), stats[4 * len(spans):].view(np.int64)
    for path, (base, total), top, n in zip(paths, spans, peak, clipped):
        wavfile.write(path, int(sr_o), host[base:base + total])
        if n:
            print(f" [Warning] {path}: {int(n)} of {total} samples clipped (peak {float(top):.3f})")


@torch.no_grad()
def run(cmd, units_encoder=None, f0_extractor=None, enhancer=None, device="cuda", batch_frames=4096,
        enhancer_batch_samples=None, units_batch_samples=None):
    """Converts `cmd.input` into `cmd.output` as the options say -> (fp64 device waveform, sample rate).  `units_encoder`,
    `f0_extractor`, `enhancer`: objects to use in place of the ones the model's config and the options name (an encoder or
    extractor built for `cmd.sampling_rate` and the model's hop at that rate).  The batching keywords are `convert_device`'s."""
    from ddsp.vocoder import F0_Extractor, Units_Encoder, load_model
    from infer_offline import convert_device
    from preprocess import load_wav

    model, args = load_model(cmd.model_path, device=device)
    sr_i = int(cmd.sampling_rate)

    def load(path):
        wave, rate = load_wav(path)
        audio = torch.from_numpy(np.ascontiguousarray(wave, dtype=np.float32)).to(device)
        if int(rate) != sr_i:
            from resample import Resample
            audio = Resample(int(rate), sr_i)(audio)
        return audio

    hop_size = int(args.data.block_size) * sr_i / int(args.data.sampling_rate)
    if f0_extractor is None:
        f0_extractor = F0_Extractor(cmd.pitch_extractor, sr_i, hop_size, float(cmd.f0_min), float(cmd.f0_max), device=device)
    if units_encoder is None:
        units_encoder = Units_Encoder(args.data.encoder, args.data.encoder_ckpt, args.data.encoder_sample_rate,
                                      args.data.encoder_hop_size, device=device)
    if enhancer is None and cmd.enhance == "true":
        from enhancer import Enhancer
        enhancer = Enhancer(args.enhancer.type, args.enhancer.ckpt, device=device)
    if getattr(cmd, "jobs", None) is not None:
        if not os.path.isdir(cmd.input):
            raise ValueError("--jobs goes with a folder as -i (and a folder as -o)")
        return _run_jobs(cmd, model, args, load, sr_i, units_encoder, f0_extractor, enhancer, device, batch_frames,
                         enhancer_batch_samples, units_batch_samples)
    if float(getattr(cmd, "formant_shift_key", 0)) != 0 or _cmd_tune(cmd) is not None or getattr(cmd, "index", None) is not None or \
            _cmd_envelope(cmd) is not None:
        return _run_formant(cmd, model, args, load, sr_i, units_encoder, f0_extractor, enhancer, device, batch_frames,
                            enhancer_batch_samples, units_batch_samples)
    if os.path.isdir(cmd.input):
        return _run_folder(cmd, model, args, load, sr_i, units_encoder, f0_extractor, enhancer, device, batch_frames,
                           enhancer_batch_samples, units_batch_samples)
    audio = load(cmd.input)
    spk_id = torch.tensor([[int(cmd.spk_id)]], dtype=torch.int64, device=device)
    result, sr_o = convert_device(model, args, audio, sr_i, None, units_encoder, f0_extractor, spk_id, batch_frames=batch_frames,
                                  key=float(cmd.key), spk_mix_dict=literal_eval(cmd.spk_mix_dict),
                                  threshold_db=float(cmd.threhold), enhancer=enhancer if cmd.enhance == "true" else None,
                                  enhancer_adaptive_key=float(cmd.enhancer_adaptive_key),
                                  enhancer_batch_samples=enhancer_batch_samples, units_batch_samples=units_batch_samples)
    _write_pcm(result, [(0, result.numel())], [cmd.output], sr_o)
    return result, sr_o


def _run_folder(cmd, model, args, load, sr_i, units_encoder, f0_extractor, enhancer, device, batch_frames, enhancer_batch_samples,
                units_batch_samples):
    """`run` for a directory: every `.wav` in `cmd.input` (sorted by name) through ONE `infer_offline.convert_many_device`, the
    results written under the same names into the directory `cmd.output` (made if missing) after one read-back of their 16-bit
    samples -> (the fp64
    device tensor holding every file, sample rate).  `-id`, `-k` and `-mix` hold for every file; a mix becomes a table row per
    file (`spk_mix_rows`).  The files are resampled to `-sr` like a single input; `-sr` must give the model an integral hop
    (`analyse_many` refuses another one)."""
    from infer_offline import convert_many_device
    names = sorted(n for n in os.listdir(cmd.input) if n.lower().endswith(".wav"))
    audios = [load(os.path.join(cmd.input, n)) for n in names]
    mix, rows = literal_eval(cmd.spk_mix_dict), None
    if mix is not None:
        rows = (torch.tensor([[int(k) for k in mix]] * len(names), dtype=torch.int32).reshape(len(names), -1).to(device),
                torch.tensor([[float(v) for v in mix.values()]] * len(names), dtype=torch.float32).reshape(len(names), -1).to(device))
    use = enhancer if cmd.enhance == "true" else None
    result, spans, sr_o = convert_many_device(
        model, args, audios, sr_i, units_encoder, f0_extractor, int(cmd.spk_id), keys=float(cmd.key), batch_frames=batch_frames,
        spk_mix_rows=rows, threshold_db=float(cmd.threhold), enhancer=use, enhancer_adaptive_key=float(cmd.enhancer_adaptive_key),
        enhancer_batch_samples=enhancer_batch_samples, units_batch_samples=units_batch_samples)
    os.makedirs(cmd.output, exist_ok=True)
    _write_pcm(result, spans, [os.path.join(cmd.output, name) for name in names], sr_o)
    return result, sr_o


def _run_formant(cmd, model, args, load, sr_i, units_encoder, f0_extractor, enhancer, device, batch_frames, enhancer_batch_samples,
                 units_batch_samples):
    """`run` with `--formant_shift_key S`, `--tune_scale`, `--index` or `--rms_mix_rate` and no `--jobs`: the file, or every `.wav` of the folder, as one job
    each - `-id` or `-mix`, `-k`, the shift and the tune - through ONE `infer_offline.convert_many_device(jobs=...)`; outputs as `run` names them."""
    from infer_offline import convert_many_device
    folder = os.path.isdir(cmd.input)
    names = sorted(n for n in os.listdir(cmd.input) if n.lower().endswith(".wav")) if folder else [None]
    audios = [load(os.path.join(cmd.input, n) if folder else cmd.input) for n in names]
    mix = literal_eval(cmd.spk_mix_dict)
    shift, tune = float(getattr(cmd, "formant_shift_key", 0)), _cmd_tune(cmd)
    files = _IndexFiles(device)
    index = files.setting("--index", getattr(cmd, "index", None), getattr(cmd, "index_ratio", 0.5))
    jobs = _file_jobs(len(names), [Job(None, 0, int(cmd.spk_id) if mix is None else mix, float(cmd.key),
                                       shift if shift != 0 else None, tune, index, _cmd_envelope(cmd))])
    result, spans, sr_o = convert_many_device(
        None, args, audios, sr_i, units_encoder, f0_extractor, jobs=jobs, models=[model], batch_frames=batch_frames,
        indices=files.bank(),
        threshold_db=float(cmd.threhold), enhancer=enhancer if cmd.enhance == "true" else None,
        enhancer_adaptive_key=float(cmd.enhancer_adaptive_key), enhancer_batch_samples=enhancer_batch_samples,
        units_batch_samples=units_batch_samples)
    if folder:
        os.makedirs(cmd.output, exist_ok=True)
    _write_pcm(result, spans, [os.path.join(cmd.output, n) for n in names] if folder else [cmd.output], sr_o)
    return result, sr_o


def _run_jobs(cmd, model, args, load, sr_i, units_encoder, f0_extractor, enhancer, device, batch_frames, enhancer_batch_samples,
              units_batch_samples):
    """`run` with `--jobs`: every entry of the list applied to every `.wav` of `cmd.input` (sorted by name), file after file and
    entry after entry, through ONE `infer_offline.convert_many_device(jobs=...)` - one analysis per file - and one read-back ->
    (the fp64 device tensor holding every output, sample rate).  The models are loaded once each, `-m` first (it is model 0 and
    gives the configuration); they must agree as `job_table` says."""
    import yaml

    from ddsp.vocoder import load_model
    from infer_offline import convert_many_device
    with open(cmd.jobs) as fh:
        entries = yaml.safe_load(fh)
    if not (isinstance(entries, list) and entries and all(isinstance(e, dict) for e in entries)):
        raise ValueError(f"--jobs: {cmd.jobs} must hold a non-empty list of {{model, id | mix, key, suffix}} entries")
    paths, models, voices, suffixes = [os.path.abspath(cmd.model_path)], [model], [], []
    shift = float(getattr(cmd, "formant_shift_key", 0))          # the shift of the entries that name none
    files = _IndexFiles(device)
    for n, e in enumerate(entries):
        spk, key = _job_entry(n, e)
        path = os.path.abspath(e.get("model", cmd.model_path))
        if path not in paths:
            paths.append(path)
            models.append(load_model(path, device=device)[0])
        index = files.setting(f"--jobs: entry {n}", e.get("index", getattr(cmd, "index", None)),
                              e.get("index_ratio", getattr(cmd, "index_ratio", 0.5)))
        suffixes.append(str(e["suffix"]))
        voices.append(Job(None, paths.index(path), spk, key, _job_formant(n, e, shift), _job_tune(n, e, _cmd_tune(cmd)), index,
                          _job_envelope(n, e, _cmd_envelope(cmd))))
    if len(set(suffixes)) != len(suffixes):
        raise ValueError("--jobs: two entries share a suffix, so they would write the same files")
    names = sorted(n for n in os.listdir(cmd.input) if n.lower().endswith(".wav"))
    audios = [load(os.path.join(cmd.input, n)) for n in names]
    jobs = _file_jobs(len(names), voices)
    out_paths = [os.path.join(cmd.output, f"{os.path.splitext(name)[0]}_{suffix}.wav") for name in names for suffix in suffixes]
    result, spans, sr_o = convert_many_device(
        None, args, audios, sr_i, units_encoder, f0_extractor, jobs=jobs, models=models, batch_frames=batch_frames,
        indices=files.bank(),
        threshold_db=float(cmd.threhold), enhancer=enhancer if cmd.enhance == "true" else None,
        enhancer_adaptive_key=float(cmd.enhancer_adaptive_key), enhancer_batch_samples=enhancer_batch_samples,
        units_batch_samples=units_batch_samples)
    os.makedirs(cmd.output, exist_ok=True)
    _write_pcm(result, spans, out_paths, sr_o)
    return result, sr_o


def _file_jobs(n_files, voices):
    """Every voice - a `Job` whose file is still None - applied to every file -> the jobs, file after file and voice after voice."""
    return [dataclasses.replace(voice, file=k) for k in range(n_files) for voice in voices]


class _IndexFiles:
    """The `UnitIndex` files a run names, each loaded once and numbered in the order it is first named; `bank()` is their
    `UnitIndexBank` on the device, None when no file was named."""

    def __init__(self, device):
        self.device, self.paths, self.indices = device, [], []

    def setting(self, where, path, ratio):
        """-> a job's seventh entry (index_number, ratio), None without a file."""
        if path is None:
            return None
        path = os.path.abspath(str(path))
        if path not in self.paths:
            self.indices.append(UnitIndex.load(path))
            self.paths.append(path)
        setting = (self.paths.index(path), float(ratio))
        check_job_index(where, setting)
        return setting

    def bank(self):
        return UnitIndexBank(self.indices, device=self.device) if self.indices else None


def _job_entry(n, e):
    """Entry n of the `--jobs` list -> (spk, key) as `infer_offline.job_table` takes them: the speaker from `id`, `mix` or
    `timeline` (at most one of them; default id 1), the key from `key` or `key_timeline` (not both; default 0).  ValueError for an
    unknown field, two speakers, two keys or a missing suffix."""
    unknown = set(e) - {"model", "id", "mix", "timeline", "key", "key_timeline", "formant", "formant_timeline", "tune", "index",
                        "index_ratio", "envelope", "suffix"}
    if unknown or sum(k in e for k in ("id", "mix", "timeline")) > 1 or ("key" in e and "key_timeline" in e) or \
            not str(e.get("suffix", "")):
        raise ValueError(f"--jobs: entry {n} takes model, id or mix or timeline, key or key_timeline and a non-empty suffix, "
                         f"got {e!r}")
    spk = _timeline(n, e["timeline"]) if "timeline" in e else e["mix"] if "mix" in e else int(e.get("id", 1))
    key = _key_timeline(n, e["key_timeline"]) if "key_timeline" in e else float(e.get("key", 0))
    return spk, key


def _job_formant(n, e, default=0.0):
    """Entry n's formant shift as a job's fifth entry: `formant: <semitones>`, `formant_timeline: [{at: <seconds>, formant:
    <semitones>}, ...]` (`infer_offline.FormantTimeline`) - not both -, else `default` (`--formant_shift_key`); None for no shift."""
    if "formant" in e and "formant_timeline" in e:
        raise ValueError(f"--jobs: entry {n} takes formant or formant_timeline, not both, got {e!r}")
    if "formant_timeline" in e:
        points = e["formant_timeline"]
        if not (isinstance(points, list) and points and all(isinstance(p, dict) and set(p) == {"at", "formant"} for p in points)):
            raise ValueError(f"--jobs: entry {n}: formant_timeline is a non-empty list of {{at, formant}} points, got {points!r}")
        return FormantTimeline([(p["at"], p["formant"]) for p in points])
    shift = float(e.get("formant", default))
    return None if shift == 0 else shift


def _tune(where, scale=None, notes=None, strength=1.0, retune_ms=50.0, a4=440.0):
    """`infer_offline.PitchTune` from a scale ('A minor') or a list of notes - one of them - with the retune time in milliseconds."""
    if (scale is None) == (notes is None):
        raise ValueError(f"{where}: a tune takes scale or notes, one of them")
    kw = {"strength": float(strength), "retune": float(retune_ms) / 1000.0, "a4": float(a4)}
    return PitchTune.named(scale, **kw) if notes is None else PitchTune(notes, **kw)


def _cmd_tune(cmd):
    """`--tune_scale` with `--tune_strength`, `--tune_retune_ms` and `--tune_a4` -> a PitchTune, None without `--tune_scale`."""
    if getattr(cmd, "tune_scale", None) is None:
        return None
    return _tune("--tune_scale", scale=cmd.tune_scale, strength=getattr(cmd, "tune_strength", 1.0),
                 retune_ms=getattr(cmd, "tune_retune_ms", 50.0), a4=getattr(cmd, "tune_a4", 440.0))


def _job_tune(n, e, default=None):
    """Entry n's pitch correction as a job's sixth entry: `tune: {scale | notes, strength, retune_ms, a4}`, else `default`
    (`--tune_scale`)."""
    if "tune" not in e:
        return default
    t = e["tune"]
    if not (isinstance(t, dict) and set(t) <= {"scale", "notes", "strength", "retune_ms", "a4"}):
        raise ValueError(f"--jobs: entry {n}: tune is {{scale | notes, strength, retune_ms, a4}}, got {t!r}")
    return _tune(f"--jobs: entry {n}", **t)


def _envelope(where, rate, hop_ms=500.0, frames=2):
    """`infer_offline.EnvelopeMix` from a rate, the hop in milliseconds and the window in hops."""
    try:
        return EnvelopeMix(float(rate), float(hop_ms) / 1000.0, frames)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{where}: {e}") from None


def _cmd_envelope(cmd):
    """`--rms_mix_rate R` -> an EnvelopeMix at RVC's offline hop and window, None without the option."""
    if getattr(cmd, "rms_mix_rate", None) is None:
        return None
    return _envelope("--rms_mix_rate", cmd.rms_mix_rate)


def _job_envelope(n, e, default=None):
    """Entry n's envelope mix as a job's eighth entry: `envelope: <rate>` or `envelope: {rate, hop_ms, frames}`, else `default`
    (`--rms_mix_rate`)."""
    if "envelope" not in e:
        return default
    v = e["envelope"]
    if isinstance(v, dict):
        if "rate" not in v or not set(v) <= {"rate", "hop_ms", "frames"}:
            raise ValueError(f"--jobs: entry {n}: envelope is a rate or {{rate, hop_ms, frames}}, got {v!r}")
        return _envelope(f"--jobs: entry {n}", **v)
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"--jobs: entry {n}: envelope is a rate or {{rate, hop_ms, frames}}, got {v!r}")
    return _envelope(f"--jobs: entry {n}", v)


def _timeline(n, points):
    """An entry's `timeline: [{at: <seconds>, id: n} | {at: <seconds>, mix: {id: weight}}, ...]` -> `SpeakerTimeline`."""
    if not (isinstance(points, list) and points and all(isinstance(p, dict) and set(p) in ({"at", "id"}, {"at", "mix"}) for p in points)):
        raise ValueError(f"--jobs: entry {n}: timeline is a non-empty list of {{at, id}} or {{at, mix}} points, got {points!r}")
    return SpeakerTimeline([(p["at"], p["id"] if "id" in p else p["mix"]) for p in points])


def _key_timeline(n, points):
    """An entry's `key_timeline: [{at: <seconds>, key: <semitones>}, ...]` -> `KeyTimeline`."""
    if not (isinstance(points, list) and points and all(isinstance(p, dict) and set(p) == {"at", "key"} for p in points)):
        raise ValueError(f"--jobs: entry {n}: key_timeline is a non-empty list of {{at, key}} points, got {points!r}")
    return KeyTimeline([(p["at"], p["key"]) for p in points])


if __name__ == "__main__":
    run(parse_args())
