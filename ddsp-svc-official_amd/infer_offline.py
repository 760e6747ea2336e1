"""The reference's offline CLI (`main.py:88-174`) restated around the device path.

The reference's `main.py` is broken as shipped (`.astype` on a tensor at :112, key shift applied twice at :105/:120,
SURVEY 0.3), so this module restates what it intends.  `render` takes analysed features and does what happens from there:
per-slice `model(...)[0]`, the volume gate multiplied into the returned signal in place, optional enhancer, silence padding /
cross-fade of slices.  `convert` starts from the raw audio: f0 (`F0_Extractor`), volume and per-slice units
(`Units_Encoder`) on the device, then `render`.  Cutting the audio into slices (`slicer.Slicer`, a librosa-based silence
detector) stays with the caller: `convert` takes the slice boundaries.
"""
import numpy as np
import torch

import hipddsp


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


@torch.no_grad()
def render(model, args, segments, f0, volume, spk_id, spk_mix_dict=None, threshold_db=-60, enhancer=None,
           enhancer_adaptive_key=0, noise_seed=None):
    """segments: list of (start_frame, units (1, Fr_seg, n_unit)) as `main.py:143-151` produces them;
    f0 (1, Fr, 1), volume (1, Fr) cover the whole file.  Returns (float64 numpy waveform, sample rate)."""
    block = int(args.data.block_size)
    sr = int(args.data.sampling_rate)
    ctx = hipddsp.context_for(f0.device)
    result = np.zeros(0)
    current = 0
    sr_o = sr
    for start, units in segments:
        n = units.size(1)
        seg_f0 = f0[:, start:start + n, :]
        seg_vol = volume[:, start:start + n]
        kw = {} if noise_seed is None else {"noise_seed": noise_seed + start}
        out = model(units, seg_f0, seg_vol, spk_id=spk_id, spk_mix_dict=spk_mix_dict, **kw)[0]
        # the gate of the WHOLE file sliced to this segment (main.py:159): dilation sees the neighbours
        gate = volume_mask(volume, threshold_db, block)[:, start * block:(start + n) * block]
        out *= gate
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


@torch.no_grad()
def convert(model, args, audio, sample_rate, slices, units_encoder, f0_extractor, spk_id, key=0, spk_mix_dict=None,
            threshold_db=-60, enhancer=None, enhancer_adaptive_key=0, noise_seed=None):
    """`main.py:88-174` from the raw audio: audio (T,) numpy array or device tensor at `sample_rate`; `slices` a list of
    (start_sample, end_sample) as the reference's `Slicer` tags them (`split_time`) - the slicer itself is not part of this
    package, any silence detector that yields sample ranges will do.  f0 of the whole file (uv_interp on) shifted by `key`
    semitones ONCE (the reference applies the shift twice), volume of the whole file at
    `hop_size = block_size * sample_rate / sampling_rate`, then per slice, snapped to whole frames as `main.split` does
    (main.py:41-46: start_frame = int(start // hop_size), end_frame = int(end // hop_size), audio[int(start_frame *
    hop_size) : int(end_frame * hop_size)], empty slices dropped), the units of that slice's audio (main.py:148-151), then
    `render`.  `units_encoder` / `f0_extractor`: `ddsp.vocoder.Units_Encoder` / `F0_Extractor` built for `sample_rate` and
    that hop (ValueError otherwise).  Returns (float64 numpy waveform, sample rate)."""
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
    segments = []
    for start, end in slices:
        start_frame, end_frame = int(int(start) // hop_size), int(int(end) // hop_size)
        if end_frame > start_frame:
            seg = x[None, int(start_frame * hop_size):int(end_frame * hop_size)]
            segments.append((start_frame, units_encoder.encode(seg, sample_rate, hop_size)))
    return render(model, args, segments, f0, volume, spk_id, spk_mix_dict=spk_mix_dict, threshold_db=threshold_db,
                  enhancer=enhancer, enhancer_adaptive_key=enhancer_adaptive_key, noise_seed=noise_seed)
