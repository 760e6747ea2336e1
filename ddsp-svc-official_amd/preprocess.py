"""Dataset preparation (the reference's `preprocess.py`) restated around the device analysers.

The reference analyses one file at a time at batch 1: volume, units, f0, then a host tail on the f0 contour
(`preprocess.py:69-102`).  Here the three analysers run on the device (`ddsp.vocoder.Volume_Extractor`, `Units_Encoder`,
`F0_Extractor`), and with `batch_samples=` a folder of utterances of different length goes through them in RAGGED groups:
the files are sorted by length, grouped (`infer_offline.group_segments`) so that a group's padded size stays inside the
budget, padded once, and analysed with `n_samples=` - every row as if alone, CREPE over the rows' real frames only.

`analyse_batch` is the part without files; `preprocess` is the folder walk with the reference's tree:
    <path>/audio/<spk>/<name>.wav  ->  <path>/f0/<spk>/<name>.npy, <path>/f0_stat/<spk>/<name>.npy,
                                       <path>/volume/<spk>/<name>.npy, <path>/units/<spk>/<name>.0.npy
an all-unvoiced file is moved to <path>/skip/<spk>/, and `gen_stats` writes the speaker-wise <path>/f0_stats.npy.
"""
import os
import shutil

import numpy as np
import torch

from infer_offline import group_segments
from sharding import stack_rows


def f0_tail(f0, use_vuv=False):
    """The host tail of the reference (`preprocess.py:80-91`) on one contour (n,) with 0 = unvoiced, in numpy as written
    there: -> (f0, lf0_mean, voiced).  lf0_mean is the mean of log f0 over the voiced frames (NaN when there are none);
    with voiced frames and not `use_vuv` the unvoiced ones are filled by np.interp between the voiced ones (ends held, no
    f0_min clamp); an all-unvoiced contour comes back unchanged with voiced=False."""
    f0 = np.array(f0, copy=True)
    unvoiced = f0 == 0
    with np.errstate(invalid="ignore"), _quiet_empty_mean():
        lf0_mean = np.mean(np.log(f0[~unvoiced]))
    voiced = bool((~unvoiced).any())
    if voiced and not use_vuv:
        f0[unvoiced] = np.interp(np.where(unvoiced)[0], np.where(~unvoiced)[0], f0[~unvoiced])
    return f0, lf0_mean, voiced


class _quiet_empty_mean:
    """np.mean of an empty selection is NaN with a RuntimeWarning; the all-unvoiced case is expected here."""

    def __enter__(self):
        import warnings
        self._w = warnings.catch_warnings()
        self._w.__enter__()
        warnings.simplefilter("ignore", RuntimeWarning)

    def __exit__(self, *exc):
        return self._w.__exit__(*exc)


def _check_lengths(lengths, sample_rate, hop_size, units_encoder, f0_extractor=None):
    """Every file must be long enough for each analyser (its `min_samples`); ValueError names the first one that is not, in
    the analyser's words (`too_short`; without them, by its minimum).  One that states no minimum (None, a stand-in, one of
    the reference's encoders) is held to the HuBERT-Soft rule at its `encoder_sample_rate`, or to the CREPE rule."""
    from ddsp import analysis

    def need(analyser, default, *args):
        if not hasattr(analyser, "min_samples"):
            return default.min_samples(), default.too_short
        lo, name = analyser.min_samples(*args), getattr(analyser, "f0_extractor", type(analyser).__name__)
        return lo, getattr(analyser, "too_short", f"are fewer than the {lo} samples that {name!r} needs")
    enc_sr = getattr(units_encoder, "encoder_sample_rate", analysis.HUBERT_RATE)
    needs = (need(analysis.Volume_Extractor(hop_size), None), need(f0_extractor, analysis.crepe_rule(sample_rate)),
             need(units_encoder, analysis.units_rule(sample_rate, enc_sr), sample_rate))
    for i, n in enumerate(lengths):
        for lo, too_short in needs:
            if n < lo:
                raise ValueError(f"waves[{i}]: {n} samples {too_short}")


def _record(f0, volume, units, use_vuv):
    f0, lf0_mean, voiced = f0_tail(f0, use_vuv)
    return {"f0": f0, "volume": volume, "units": units, "lf0_mean": lf0_mean, "voiced": voiced}


def analyse_batch(waves, f0_extractor, volume_extractor, units_encoder, sample_rate, hop_size, batch_samples=None,
                  use_vuv=False, *, device=None):
    """waves: a list of 1-D float arrays or tensors at `sample_rate` -> one record per input, in input order:
    {"f0" (n,), "volume" (n,), "units" (n, C)} as numpy, trimmed to the file's own n = int(len // hop_size) + 1 frames, plus
    "lf0_mean" and "voiced" (`f0_tail`).

    batch_samples=None: one file after the other through the rectangular calls at batch 1, like the reference.
    batch_samples=N: the files are sorted by length and grouped so that rows * longest <= N samples (a longer file is a
    group of its own); each group is padded once and analysed with `n_samples=`, so every row comes out as if it had been
    analysed alone.  The f0 dither (on by default, as in the reference's torchcrepe call) draws per call, so f0 differs
    between the two paths within the dither's +-20 cents; volume and units do not depend on the path beyond rounding.
    `device`: where the waves are analysed (default: the f0 extractor's).  A file too short for an analyser raises
    ValueError naming its index, before anything is launched."""
    if device is None:
        device = getattr(f0_extractor, "device", "cuda")
    xs = [torch.as_tensor(np.ascontiguousarray(w, dtype=np.float32) if isinstance(w, np.ndarray) else w).reshape(-1)
          for w in waves]
    lengths = [int(x.shape[0]) for x in xs]
    _check_lengths(lengths, sample_rate, hop_size, units_encoder, f0_extractor)
    n_out = [int(n // hop_size) + 1 for n in lengths]
    records = [None] * len(xs)
    if batch_samples is None:
        for i, x in enumerate(xs):
            x = x.to(device=device, dtype=torch.float32).reshape(1, -1)
            volume = volume_extractor.extract(x)
            units = units_encoder.encode(x, sample_rate, hop_size)
            f0 = f0_extractor.extract(x, uv_interp=False)
            records[i] = _record(f0[0, :n_out[i]].cpu().numpy(), volume[0, :n_out[i]].cpu().numpy(),
                                 units[0, :n_out[i]].cpu().numpy(), use_vuv)
        return records
    for group in group_segments(lengths, int(batch_samples)):
        x, counts = stack_rows([xs[i].to(device=device, dtype=torch.float32) for i in group])
        volume = volume_extractor.extract(x, n_samples=counts).cpu().numpy()
        units = units_encoder.encode(x, sample_rate, hop_size, n_samples=counts).cpu().numpy()
        f0 = f0_extractor.extract(x, uv_interp=False, n_samples=counts).cpu().numpy()
        for j, i in enumerate(group):
            records[i] = _record(f0[j, :n_out[i]], volume[j, :n_out[i]].copy(), units[j, :n_out[i]].copy(), use_vuv)
    return records


def load_wav(path):
    """path -> (float32 mono (T,), rate) with scipy.io.wavfile: integer PCM is scaled to [-1, 1), channels are averaged."""
    from scipy.io import wavfile
    rate, data = wavfile.read(path)
    if data.dtype.kind == "i":
        data = data.astype(np.float32) / float(-np.iinfo(data.dtype).min)
    elif data.dtype.kind == "u":     # 8-bit PCM is unsigned with its zero at 128
        data = (data.astype(np.float32) - 128.0) / 128.0
    data = data.astype(np.float32)
    return (data.mean(axis=1).astype(np.float32) if data.ndim == 2 else data), int(rate)


def list_audio(srcdir, extension="wav"):
    """Paths below `srcdir`, relative to it, of the files with `extension`, sorted (hidden files left out)."""
    out = []
    for root, _, files in os.walk(srcdir):
        for f in files:
            if f.endswith("." + extension) and not f.startswith("."):
                out.append(os.path.relpath(os.path.join(root, f), srcdir))
    return sorted(out)


def preprocess(path, f0_extractor, volume_extractor, units_encoder, sample_rate, hop_size, device="cuda", gen_stats=False,
               use_vuv=False, batch_samples=None, load=None, chunk_files=256):
    """Analyses every <path>/audio/**/*.wav into the reference's tree (module docstring) through `analyse_batch`;
    `batch_samples` as there.  Returns the relative paths that were moved to skip/ (all unvoiced).

    `load(path) -> (float32 mono (T,), rate)` defaults to `load_wav` (scipy.io.wavfile).  A file at another rate than
    `sample_rate` is resampled on the device with `resample.Resample` (windowed sinc, Hann, width 6).  The reference loads
    with librosa, which resamples with its own filter (soxr), so such files are NOT sample-identical to the reference's;
    files already at `sample_rate` are.  `chunk_files` bounds how many files are held in memory at once."""
    load = load_wav if load is None else load
    src = os.path.join(path, "audio")
    dirs = {k: os.path.join(path, k) for k in ("units", "f0", "f0_stat", "volume", "skip")}
    rels = list_audio(src)
    skipped = []
    for c0 in range(0, len(rels), int(chunk_files)):
        chunk = rels[c0:c0 + int(chunk_files)]
        waves = []
        for rel in chunk:
            wave, rate = load(os.path.join(src, rel))
            if int(rate) != int(sample_rate):
                from resample import Resample
                wave = Resample(int(rate), int(sample_rate))(torch.from_numpy(np.ascontiguousarray(wave)).to(device)).cpu().numpy()
            waves.append(wave)
        records = analyse_batch(waves, f0_extractor, volume_extractor, units_encoder, sample_rate, hop_size, batch_samples,
                                use_vuv, device=device)
        for rel, rec in zip(chunk, records):
            stem = os.path.splitext(rel)[0]
            for k in ("units", "f0", "f0_stat", "volume"):
                os.makedirs(os.path.dirname(os.path.join(dirs[k], rel)), exist_ok=True)
            # (the reference writes the units before it looks at the f0, so a skipped file keeps its units)
            np.save(os.path.join(dirs["units"], stem + ".0.npy"), rec["units"])
            if rec["voiced"]:
                np.save(os.path.join(dirs["f0"], stem + ".npy"), rec["f0"])
                np.save(os.path.join(dirs["f0_stat"], stem + ".npy"), rec["lf0_mean"])
                np.save(os.path.join(dirs["volume"], stem + ".npy"), rec["volume"])
            else:
                dst = os.path.dirname(os.path.join(dirs["skip"], rel))
                os.makedirs(dst, exist_ok=True)
                shutil.move(os.path.join(src, rel), dst)
                print(f"[preprocess] no voiced frame in {os.path.join(src, rel)}: moved to {dst}")
                skipped.append(rel)
    if gen_stats:
        # speaker-wise mean of the files' mean log f0 (a mean of means, as in the reference)
        stats = {}
        if os.path.isdir(dirs["f0_stat"]):
            for spk in sorted(os.listdir(dirs["f0_stat"])):
                d = os.path.join(dirs["f0_stat"], spk)
                if os.path.isdir(d):
                    means = [np.load(os.path.join(r, f)) for r, _, fs in sorted(os.walk(d)) for f in sorted(fs) if f.endswith(".npy")]
                    if means:
                        stats[spk] = sum(means) / len(means)
        np.save(os.path.join(path, "f0_stats"), stats)
    return skipped


if __name__ == "__main__":
    import argparse

    import yaml

    from ddsp.vocoder import DotDict, F0_Extractor, Units_Encoder, Volume_Extractor

    parser = argparse.ArgumentParser(description="analyse data.train_path and data.valid_path of a training config")
    parser.add_argument("-c", "--config", type=str, required=True, help="path to the config file")
    parser.add_argument("--batch-samples", type=int, default=None,
                        help="padded samples per ragged group (default: one file at a time)")
    args = parser.parse_args()
    with open(args.config, "r") as fh:
        d = DotDict(yaml.safe_load(fh)).data
    f0_extractor = F0_Extractor(d.f0_extractor, d.sampling_rate, d.block_size, d.f0_min, d.f0_max)
    volume_extractor = Volume_Extractor(d.block_size)
    units_encoder = Units_Encoder(d.encoder, d.encoder_ckpt, d.encoder_sample_rate, d.encoder_hop_size, device="cuda")
    common = dict(use_vuv=bool(d.get("use_vuv", False)), batch_samples=args.batch_samples)
    preprocess(d.train_path, f0_extractor, volume_extractor, units_encoder, d.sampling_rate, d.block_size, gen_stats=True, **common)
    preprocess(d.valid_path, f0_extractor, volume_extractor, units_encoder, d.sampling_rate, d.block_size, **common)
