"""Drop-in for the analysis half of the reference's `ddsp/vocoder.py` (:18-229): `Volume_Extractor`, `F0_Extractor`,
`Units_Encoder`, `Audio2HubertSoft`, `Audio2CVec`, `Audio2CVec768`, plus `align_units`, executed by hand-written gfx950 kernels through libddsp_amd (no CPU
fallback).  `ddsp.vocoder` re-exports every name, so `from ddsp.vocoder import F0_Extractor` keeps working.

What the three analysers share is written once here: `_batch_of` (numpy / (T,) / (B, T) in, the caller's rank and type
out) and `_RowRule` (how short is too short: one rule per analyser, behind its ragged refusal, its solo refusal, its
`min_samples` and the refusal of a file in `preprocess`).  A solo call is the ragged call without counts.
"""
import os

import torch

import hipddsp

from .crepe import HOP as CREPE_HOP, SAMPLE_RATE as CREPE_RATE, Crepe
from .hubert import SAMPLE_RATE as HUBERT_RATE, RaggedCounts


def _batch_of(name, audio, device):
    """numpy (T,), tensor (T,) or tensor (B, T) -> ((B, T) on the device, `restore`): a numpy array is copied to `device`;
    `restore(out)` gives the result the caller's rank back, and its type (a numpy array: one synchronisation)."""
    import numpy as np
    is_np = isinstance(audio, np.ndarray)
    x = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).to(device) if is_np else audio
    if not x.is_cuda:
        raise RuntimeError(f"{name} runs on a HIP device only (no CPU fallback)")
    if x.dim() not in (1, 2):
        raise ValueError(f"{name}.extract: audio must be (T,) or (B, T)")
    flat = x.dim() == 1

    def restore(out):
        out = out[0] if flat else out
        return out.cpu().numpy() if is_np else out
    return (x.reshape(1, -1) if flat else x), restore


def _hip_device(name, device):
    """`device`, or the current HIP device for None; anything else is refused (there is no CPU fallback)."""
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError(f"{name} runs on a HIP device only (no CPU fallback)")
        return "cuda"
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"{name} runs on a HIP device only (no CPU fallback); got device=%r" % (device,))
    return device


def _ragged_batch(name, audio):
    if not isinstance(audio, torch.Tensor) or audio.dim() != 2:
        raise ValueError(f"{name}: a ragged batch is a (B, T) tensor")
    return audio.shape


class _RowRule:
    """How short is too short for one analyser, stated once.  `rule` is one of hipddsp's (`check_n_samples(..., rule)`): a
    count at the analyser's working rate -> None, or the reason a row of that many samples is too short.  Rows arrive at
    `sample_rate` and are analysed at `rate` (None: as they arrive).  `too_short` says it for a whole file
    ("<n> samples <too_short>": `preprocess`); a "{min}" in it stands for `min_samples()`, worked out when it is read."""

    def __init__(self, rule, too_short, sample_rate=None, rate=None):
        self.rule, self._too_short, self.sample_rate, self.rate = rule, too_short, sample_rate, rate

    too_short = property(lambda self: self._too_short.format(min=self.min_samples()) if "{min}" in self._too_short else self._too_short)

    def at(self, n):
        """n samples as they arrive -> samples at the working rate."""
        return n if self.rate is None else hipddsp.resample_length(n, self.sample_rate, self.rate)

    def min_samples(self):
        """The shortest row the analyser accepts, in samples as they arrive."""
        n = 1
        while self.rule(self.at(n)) is not None:
            n += 1
        return n

    def counts(self, n_samples, B, T):
        """The counts of a ragged (B, T) batch, checked on the host before anything is launched -> (counts as they arrive,
        counts at the working rate, T at the working rate)."""
        vals = hipddsp.check_n_samples(n_samples, B, T)
        T_work = self.at(T)
        return vals, hipddsp.check_n_samples([self.at(v) for v in vals], B, T_work, self.rule), T_work

    def require(self, name, T):
        """The solo refusal: a (B, T) batch whose every row has all T samples."""
        reason = self.rule(self.at(T))
        if reason is not None:
            raise ValueError(f"{name}: {self.at(T)} {reason}")


def volume_rule(hop_size):
    """The volume's rule: longer than the reflect padding."""
    return _RowRule(hipddsp.volume_rule(int(hop_size)),
                    f"are not longer than the volume's reflect padding {(int(hop_size) + 1) // 2}")


def units_rule(sample_rate, encoder_sample_rate=HUBERT_RATE, padded=True):
    """The units encoder's rule for rows at `sample_rate`: HuBERT-Soft's, which pads 40 samples on each side, or with
    `padded=False` that of the base form ('cvec', 'cvec768'), which does not."""
    return _RowRule(hipddsp.hubert_rule if padded else hipddsp.hubert_base_rule,
                    "are too short for the units encoder's conv stack", sample_rate, encoder_sample_rate)


def crepe_rule(sample_rate):
    """The CREPE rule for rows at `sample_rate`: at least 3 CREPE frames."""
    return _RowRule(hipddsp.crepe_rule(CREPE_HOP), "give fewer than 3 CREPE frames", sample_rate, CREPE_RATE)


def ac_rule(sample_rate, hop_size, f0_min):
    """The rule of the autocorrelation f0 extractor: one analysis window of 3 / f0_min seconds."""
    return _RowRule(hipddsp.f0_ac_rule(sample_rate, hop_size, f0_min),
                    "are shorter than one analysis window of the 'ac' f0 extractor ({min} samples)")


class Volume_Extractor:
    """Frame RMS of an audio signal on the device (reference `ddsp/vocoder.py:116-137`, same constructor and method).

    `extract(audio)`: a numpy array (T,) as the reference's callers pass (`main.py`, `preprocess.py`) comes back as a
    numpy array (Frame,) - it is copied to `device`, reduced there and copied back; a device tensor (T,) or (B,T)
    comes back as a device tensor of the same rank.  There is no CPU computation path."""

    def __init__(self, hop_size=512, device="cuda"):
        self.hop_size = hop_size
        self.device = device

    too_short = property(lambda self: volume_rule(self.hop_size).too_short)

    def min_samples(self):
        """The shortest row `extract(..., n_samples=)` accepts."""
        return volume_rule(self.hop_size).min_samples()

    def extract(self, audio, n_samples=None):
        """`n_samples` (a sequence of B ints or a CPU integer tensor (B,), each > (hop_size + 1) // 2; device tensor (B,T) and
        an integral hop only): a RAGGED batch - row b reflects at its own ends, carries n_samples[b] // hop_size + 1 frames
        and is 0 after them, and what follows its samples may hold anything."""
        # an integral hop (int or float) takes the integer entry point; block_size * sr / model_sr of an input at another
        # rate than the model's (main.py:72,109) is fractional and keeps its fraction, as the reference's float slicing does
        hop = int(self.hop_size) if float(self.hop_size).is_integer() else float(self.hop_size)
        if n_samples is not None:
            B, T = _ragged_batch("Volume_Extractor.extract", audio)
            if not isinstance(hop, int):
                raise ValueError("Volume_Extractor.extract: a ragged batch needs an integral hop_size")
            n_samples = hipddsp.check_volume_n_samples(n_samples, B, T, hop)     # (before any launch)
        x, restore = _batch_of("Volume_Extractor", audio, self.device)
        return restore(hipddsp.context_for(x.device).volume_extract(x, hop, n_samples))


def _find_torchcrepe_checkpoint(model="full"):
    """`assets/<model>.pth` of an installed torchcrepe, located with importlib.util.find_spec (the package is not imported)."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torchcrepe")
    except (ImportError, ValueError):
        spec = None
    for d in (list(spec.submodule_search_locations or []) if spec is not None else []):
        p = os.path.join(d, "assets", f"{model}.pth")
        if os.path.isfile(p):
            return p
    raise FileNotFoundError(
        f"F0_Extractor('crepe'): no CREPE checkpoint given and no installed torchcrepe with assets/{model}.pth was found; pass "
        "crepe_ckpt='/path/to/full.pth' (torchcrepe's state dict) or a ddsp.crepe.Crepe module")


class _CrepeF0:
    """The 'crepe' back end of `F0_Extractor`: resampling to 16 kHz, the network over the rows' own frames, the Viterbi decode
    with its dither, and the reference's post-filter."""
    dithers = True      # (`seed_dev` means something to it: refused with a ragged batch)

    def __init__(self, sample_rate, hop_size, f0_min, f0_max, crepe_ckpt, device):
        self.sample_rate, self.hop_size, self.f0_min, self.f0_max = sample_rate, hop_size, f0_min, f0_max
        self.rule = crepe_rule(sample_rate)
        if isinstance(crepe_ckpt, Crepe):
            model = crepe_ckpt
        else:
            path = crepe_ckpt if crepe_ckpt is not None else _find_torchcrepe_checkpoint("full")
            sd = torch.load(path, map_location="cpu", weights_only=True)
            model = Crepe("tiny" if sd["conv1.weight"].shape[0] == 128 else "full")
            model.load_state_dict(sd)
        self.model = model.to(device).eval()

    def run(self, ctx, x, counts, n_frames, start_frame, uv_interp, dither, seed, seed_dev):
        """x (B, T) fp32 on the device; `counts`: None, or `self.rule.counts(...)` of a ragged batch -> f0 (B, n_frames)."""
        sr, hop = self.sample_rate, self.hop_size
        n_dev, rows, decode, post = None, (), {}, {}
        if counts is not None:
            vals, n16, _ = counts
            B = len(vals)
            n_crepe = [hipddsp.crepe_frames(v, CREPE_HOP) for v in n16]
            n_out = [int(v // hop) + 1 for v in vals]
            # one upload: the rows' samples, the activations' table (16 kHz samples, frame prefix), CREPE frames, output frames
            dev = ctx.ragged_counts(vals + hipddsp.crepe_ragged_table(n16, CREPE_HOP) + n_crepe + n_out)
            n_dev, table_dev, nc_dev, no_dev = dev[:B], dev[B:3 * B + 1], dev[3 * B + 1:4 * B + 1], dev[4 * B + 1:]
            rows, decode = (n16, table_dev), dict(n_frames=n_crepe, counts_dev=nc_dev)
            post = dict(n_crepe=n_crepe, n_out=n_out, counts_dev=(nc_dev, no_dev))
        x16 = x if int(sr) == CREPE_RATE else ctx.resample(x, int(sr), CREPE_RATE, lowpass_filter_width=128, n_dev=n_dev)
        probs = self.model.activations(x16, CREPE_HOP, *rows)
        if seed_dev is not None:
            f0, pd = ctx.crepe_decode(probs, self.f0_min, self.f0_max, segment=512, dither=dither, seed_dev=seed_dev)
        else:
            if dither and seed is None:
                seed = hipddsp.seed_from_torch()
            f0, pd = ctx.crepe_decode(probs, self.f0_min, self.f0_max, segment=512, dither_seed=int(seed or 0), dither=dither,
                                      **decode)
        return ctx.f0_postfilter(f0, pd, sr, hop, n_frames, start_frame, 0.05, uv_interp, self.f0_min, **post)


class _AcF0:
    """The 'ac' back end of `F0_Extractor`: the autocorrelation method in one launch.  No weights, no resampling, no
    randomness: the dither arguments are accepted and ignored."""
    model, dithers = None, False

    def __init__(self, sample_rate, hop_size, f0_min, f0_max, crepe_ckpt=None, device=None):
        if not float(f0_max) > float(f0_min) > 0:
            raise ValueError("F0_Extractor('ac'): needs 0 < f0_min < f0_max")
        self.sample_rate, self.hop_size, self.f0_min, self.f0_max = sample_rate, hop_size, f0_min, f0_max
        self.rule = ac_rule(sample_rate, hop_size, f0_min)

    def run(self, ctx, x, counts, n_frames, start_frame, uv_interp, dither=None, seed=None, seed_dev=None):
        n_dev = None if counts is None else ctx.ragged_counts(counts[0])
        return ctx.f0_ac(x, self.sample_rate, self.hop_size, self.f0_min, self.f0_max, n_frames, start_frame, uv_interp,
                         n_dev=n_dev)


class F0_Extractor:
    """Reference `ddsp/vocoder.py:18-113` for `f0_extractor='crepe'`: resampling to 16 kHz (`ddsp_resample`,
    lowpass_filter_width=128), the CREPE network, the Viterbi decode and the reference's post-filter, all on the device.

    `extract(audio, uv_interp=False, device=None, silence_front=0)`: a numpy array (T,) returns a numpy fp32 array
    (n_frames,) like the reference's (one synchronisation); a device tensor (T,) or (B,T) returns a device tensor (n_frames,)
    or (B, n_frames) without a host synchronisation, so the call can be captured into a HIP graph.
    Differences a caller can observe, all additive:
      * keyword arguments `crepe_ckpt` (a path to torchcrepe's `full.pth` / `tiny.pth` state dict, or a `ddsp.crepe.Crepe`;
        None looks for an installed torchcrepe's `assets/full.pth`) and `device` (default: the current HIP device);
      * `extract(..., dither=True, seed=None)`: torchcrepe dithers the decoded pitch by a random triangular offset of up to
        +-20 cents (a bin is 20 cents); `dither=False` makes the output deterministic, `seed` fixes the draw (default: drawn
        from torch's generator); `seed_dev` (a (1,) int64 device tensor) holds the seed on the device instead and is advanced
        by every call (`seed_dev` of `ddsp_crepe_decode`), so a call captured into a HIP graph dithers anew on every replay;
      * `extract(audio (B,T), ..., n_samples=)`: a RAGGED batch of rows of different length (see `extract`);
      * 'parselmouth', 'dio' and 'harvest' (CPU libraries) raise NotImplementedError;
      * `f0_extractor='ac'`: the autocorrelation method of Boersma (1993) on the device (`ddsp_f0_ac`) - the algorithm behind
        the reference's 'parselmouth' branch (Praat's `to_pitch_ac`) with that branch's parameters (voicing threshold 0.6,
        the window of 3 / f0_min seconds, its padding to n_frames), restated from the paper's formulae.  It carries its own
        name because Praat is not a dependency and agreement with Praat itself is not pinned.  No weights, no resampling, no
        randomness: `dither`, `seed` and `seed_dev` are accepted and ignored.  Same `extract` contract as 'crepe' (numpy in,
        numpy out; device tensors without a host synchronisation; `n_samples=` ragged rows, each of at least one window)
        with the reference's treatment of unvoiced frames: 0 without `uv_interp`, interpolated and clamped to f0_min with it
        (an all-unvoiced signal becomes all f0_min).
    What differs between the two lives in a back end (`_CrepeF0`, `_AcF0`): construction, the row-length rule and `run`."""

    _BACK_ENDS = {'crepe': _CrepeF0, 'ac': _AcF0}

    def __init__(self, f0_extractor, sample_rate=44100, hop_size=512, f0_min=65, f0_max=800, *, crepe_ckpt=None, device=None):
        if f0_extractor in ('parselmouth', 'dio', 'harvest'):
            raise NotImplementedError(
                f"f0 extractor '{f0_extractor}' has no device implementation (it is a CPU library): 'crepe' is the device "
                "extractor; keep the reference's F0_Extractor for the others")
        if f0_extractor not in self._BACK_ENDS:
            raise ValueError(f" [x] Unknown f0 extractor: {f0_extractor}")
        self.f0_extractor, self.sample_rate, self.hop_size, self.f0_min, self.f0_max = \
            f0_extractor, sample_rate, hop_size, f0_min, f0_max
        self.device = _hip_device("F0_Extractor", device)
        self.back_end = self._BACK_ENDS[f0_extractor](sample_rate, hop_size, f0_min, f0_max, crepe_ckpt, self.device)
        self.model = self.back_end.model

    too_short = property(lambda self: self.back_end.rule.too_short)

    def min_samples(self):
        """The shortest row `extract` accepts, in samples at `sample_rate`."""
        return self.back_end.rule.min_samples()

    def extract(self, audio, uv_interp=False, device=None, silence_front=0, *, dither=True, seed=None, seed_dev=None,
                n_samples=None):
        """audio (T,) numpy / (T,) or (B,T) device tensor at `sample_rate` -> f0 [Hz] (n_frames,) / (B, n_frames),
        n_frames = int(T // hop_size) + 1.  `device` is accepted for the reference's signature (the model's device is used).
        `n_samples` (a sequence of B ints or a CPU integer tensor (B,), counts at `sample_rate`; device tensor (B,T) only): a
        RAGGED batch.  Row b is analysed as audio[b, :n_samples[b]] alone - resampling, framing, decode and post-filter
        each stop at the row's own end, the network computes the rows' own frames only, and what follows a row's samples may
        hold anything.  Returns (B, int(max(n_samples) // hop_size) + 1); row b carries int(n_samples[b] // hop_size) + 1
        frames and zeros after them.  Every row must be at least `min_samples()` long (3 CREPE frames; one analysis window
        of 'ac'); `silence_front != 0` and, with 'crepe', `seed_dev` are not available with it (ValueError)."""
        sr, hop, rule = self.sample_rate, self.hop_size, self.back_end.rule
        counts, start_frame, crop = None, 0, 0
        if n_samples is not None:
            if silence_front != 0:
                raise ValueError("F0_Extractor.extract: silence_front is not available with n_samples (a ragged batch)")
            if seed_dev is not None and self.back_end.dithers:
                raise ValueError("F0_Extractor.extract: seed_dev is not available with n_samples (a ragged batch)")
            counts = rule.counts(n_samples, *_ragged_batch("F0_Extractor.extract", audio))     # (before any launch)
        x, restore = _batch_of("F0_Extractor", audio, self.device)
        if counts is None:
            n_frames = int(x.shape[-1] // hop) + 1
            start_frame = int(silence_front * sr / hop)
            real_silence_front = start_frame * hop / sr
            crop = int(round(real_silence_front * sr))
            rule.require(f"F0_Extractor('{self.f0_extractor}')", x.shape[-1] - crop)
        else:
            n_frames = int(max(counts[0]) // hop) + 1
        x = x[:, crop:].contiguous().float()
        return restore(self.back_end.run(hipddsp.context_for(x.device), x, counts, n_frames, start_frame, uv_interp, dither,
                                         seed, seed_dev))


def align_units(units, n_samples, sample_rate, hop_size, encoder_sample_rate=16000, encoder_hop_size=320):
    """Nearest-frame alignment of encoder units (B, Lu, C) to the synthesiser's frames - the tail of the reference's
    `Units_Encoder.encode` (`ddsp/vocoder.py:201-211`), for callers that keep the reference's encoders and want the
    gather on the device: n_frames = int(n_samples // hop_size) + 1 (a float hop keeps its fraction, like the
    reference's), row i takes unit min(round(ratio * i), Lu - 1)."""
    n_frames = int(int(n_samples) // hop_size) + 1
    ratio = (hop_size / sample_rate) / (encoder_hop_size / encoder_sample_rate)
    return hipddsp.context_for(units.device).align_units(units, n_frames, ratio)


class Audio2HubertSoft(torch.nn.Module):
    """Reference `ddsp/vocoder.py:214-229`: the HuBERT-Soft checkpoint (`module.` prefix stripped) behind `forward(audio (B,T))
    -> units (B, Frame, 256)`, executed by libddsp_amd (`ddsp.hubert.HubertSoft`).  The module is built on `device` (default:
    the current HIP device) because there is no CPU execution path."""

    def __init__(self, path, h_sample_rate=16000, h_hop_size=320, device=None):
        super().__init__()
        from torch.nn.modules.utils import consume_prefix_in_state_dict_if_present
        from .hubert import HubertSoft
        print(' [Encoder Model] HuBERT Soft')
        self.hubert = HubertSoft()
        print(' [Loading] ' + path)
        checkpoint = torch.load(path, map_location="cpu")
        consume_prefix_in_state_dict_if_present(checkpoint, "module.")
        self.hubert.load_state_dict(checkpoint)
        self.hubert.eval()
        if device is not None:
            self.hubert.to(device)

    def forward(self, audio, n_samples=None):
        """ :: (B, T) -> (B, 1, T) -> (B, Frame, Feat=256); `n_samples`: ragged batch (`HubertSoft.units`) """
        return self.hubert.units(audio.unsqueeze(1), n_samples)


class _Audio2Base(torch.nn.Module):
    """A fairseq HuBERT-base checkpoint (`ddsp.hubert.read_fairseq_checkpoint`: a plain state dict, or one under "model")
    behind `forward(audio (B,T)) -> units (B, Frame, n_unit)`, executed by libddsp_amd (`ddsp.hubert.HubertBase`): transformer
    layer 9, as every base-form class of the reference (`ddsp/vocoder.py:231-332`).  Unlike the reference's ContentVec
    classes, whose `view(1, -1)` glues a batch into one row, every row is encoded on its own and every row is returned."""
    n_unit, project, label = None, None, None

    def __init__(self, path, h_sample_rate=16000, h_hop_size=320, device=None):
        super().__init__()
        from .hubert import HubertBase, read_fairseq_checkpoint
        print(' [Encoder Model] ' + self.label)
        self.hubert = HubertBase()
        print(' [Loading] ' + path)
        self.hubert.load_state_dict(read_fairseq_checkpoint(path))
        self.hubert.eval()
        if device is not None:
            self.hubert.to(device)

    def forward(self, audio, n_samples=None):
        """ :: (B, T) -> (B, 1, T) -> (B, Frame, n_unit); `n_samples`: ragged batch (`HubertBase.units`) """
        return self.hubert.units(audio.unsqueeze(1), n_samples, layer=9, project=self.project)


class Audio2CVec(_Audio2Base):
    """'cvec': layer 9 then `final_proj`, 256 channels - what the reference's `Audio2ContentVec` and `Audio2HubertBase`
    compute (the two differ in the checkpoint only)."""
    n_unit, project, label = 256, True, "HuBERT-base / ContentVec, layer 9, final_proj (256)"


class Audio2CVec768(_Audio2Base):
    """'cvec768': the layer-9 hidden state, 768 channels - the reference's `Audio2ContentVec768` and `Audio2HubertBase768`."""
    n_unit, project, label = 768, False, "HuBERT-base / ContentVec, layer 9 (768)"


def check_units_width(name, units_encoder, *models):
    """The encoder's channels against every model's `n_unit`, before anything is launched: ValueError on a mismatch.  An
    encoder that does not state its width (a stand-in), or a model without `unit2ctrl`, is not checked."""
    width = getattr(units_encoder, "n_unit", None)
    for m in models:
        n_unit = getattr(getattr(m, "unit2ctrl", None), "n_unit", None)
        if width is not None and n_unit is not None and int(width) != int(n_unit):
            raise ValueError(f"{name}: the units encoder '{getattr(units_encoder, 'encoder', '?')}' gives {int(width)} channels "
                             f"and the model was built for n_unit = {int(n_unit)} (config: encoder_out_channels)")


MODEL_FIELDS = ("sampling_rate", "block_size", "n_unit", "device")      # what the models of one call, or of one bank, agree in


def _model_field(model, field):
    if field == "n_unit":
        return int(model.unit2ctrl.n_unit)
    if field == "device":
        return next(model.parameters()).device
    host = getattr(model, {"sampling_rate": "_sr", "block_size": "_hop"}[field], None)   # (the synthesisers' host copies:
    return int(getattr(model, field) if host is None else host)                          # the buffers would be read back)


class Units_Encoder:
    """Reference `ddsp/vocoder.py:140-211` for `encoder='hubertsoft'`: resampling to the encoder's rate (`ddsp_resample`,
    lowpass_filter_width=128, as the reference's torchaudio Resample), the encoder and the nearest-frame alignment
    (`align_units`), all on the device.

    Differences a caller can observe, all additive: audio (B,T) with B > 1 returns every row aligned (the reference
    returns row 0 only); the other encoder names raise NotImplementedError - `hubertsoft` is the device encoder, and callers
    that keep the reference's encoders can align their units on the device with `align_units`.

    `encoder='cvec'` / `'cvec768'`: fairseq's HuBERT-base network (ContentVec and HuBERT-base checkpoints) on the device, layer
    9 with `final_proj` (256 channels) or without (768) - what the reference computes under 'contentvec' / 'hubertbase' and
    'contentvec768' / 'hubertbase768'.  They carry names of their own because the reference's names keep raising here (fairseq
    is no dependency, and loading a released checkpoint file is not pinned by a test).  Resampler, alignment and ragged
    batches are those of 'hubertsoft'; the frame rule is the encoder's own (no padding: 400 samples at 16 kHz give the first
    frame), and every row of a batch is encoded on its own (the reference's ContentVec classes glue a batch into one row).
    `n_unit`: the channels of `encode`'s result."""

    # encoder -> (module, channels, whether the encoder pads its input)
    _MODELS = {'hubertsoft': (Audio2HubertSoft, 256, True), 'cvec': (Audio2CVec, 256, False), 'cvec768': (Audio2CVec768, 768, False)}
    encoder, n_unit, padded = 'hubertsoft', 256, True        # (of an instance made without the constructor)

    def __init__(self, encoder, encoder_ckpt, encoder_sample_rate=16000, encoder_hop_size=320, device=None):
        if encoder in ('hubertbase', 'hubertbase768', 'contentvec', 'contentvec768', 'xunit', 'yunit'):
            hint = "" if encoder in ('xunit', 'yunit') else (
                f"  The network behind '{encoder}' runs on the device as '{'cvec768' if encoder.endswith('768') else 'cvec'}' "
                "('cvec': layer 9 and final_proj, 256 channels; 'cvec768': layer 9, 768 channels), given the fairseq "
                "checkpoint's state dict.")
            raise NotImplementedError(
                f"units encoder '{encoder}' has no device implementation under that name: 'hubertsoft' is the device encoder "
                "of the reference's names; callers that keep the reference's encoders can align their units on the device with "
                "ddsp.vocoder.align_units." + hint)
        if encoder not in self._MODELS:
            raise ValueError(f" [x] Unknown units encoder: {encoder}")
        cls, self.n_unit, self.padded = self._MODELS[encoder]
        self.encoder = encoder
        self.device = _hip_device("Units_Encoder", device)
        self.model = cls(encoder_ckpt, device=self.device).eval()
        self.encoder_sample_rate = encoder_sample_rate
        self.encoder_hop_size = encoder_hop_size

    too_short = units_rule(None).too_short

    def rule(self, sample_rate):
        """This encoder's row-length rule for rows at `sample_rate`."""
        return units_rule(sample_rate, self.encoder_sample_rate, self.padded)

    def min_samples(self, sample_rate):
        """The shortest row `encode` accepts, in samples at `sample_rate`."""
        return self.rule(sample_rate).min_samples()

    def encode(self, audio, sample_rate, hop_size, n_samples=None):
        """audio (B,T) at `sample_rate` -> units (B, int(T // hop_size) + 1, n_unit) aligned to frames of `hop_size` samples
        (a float hop keeps its fraction, like the reference's).
        `n_samples` (a sequence of B ints or a CPU integer tensor (B,), counts at `sample_rate`): a RAGGED batch.  Row b is
        encoded as audio[b, :n_samples[b]] alone - resampling, encoder and alignment each stop at the row's own end, and
        what follows a row's samples may hold anything.  Returns (B, int(max(n_samples) // hop_size) + 1, n_unit); row b
        carries int(n_samples[b] // hop_size) + 1 frames and zeros after them."""
        enc_sr = self.encoder_sample_rate
        if n_samples is not None:
            if audio.dim() != 2:
                raise ValueError("Units_Encoder.encode: a ragged batch is (B, T) audio")
            vals, n16, T16 = self.rule(sample_rate).counts(n_samples, *audio.shape)     # (before any launch)
        if not audio.is_cuda:
            raise RuntimeError("Units_Encoder runs on a HIP device only (no CPU fallback)")
        ctx = hipddsp.context_for(audio.device)
        n_dev, rows, n_frames, aligned = None, None, int(audio.size(-1) // hop_size) + 1, {}
        if n_samples is not None:
            n_out = [int(v // hop_size) + 1 for v in vals]
            # one upload for the four count vectors
            frames = hipddsp.hubert_frames if self.padded else hipddsp.hubert_base_frames
            dev = ctx.ragged_counts(vals + n16 + [frames(v) for v in n16] + n_out).reshape(4, -1)
            n_dev, rows, n_frames = dev[0], RaggedCounts(n16, T16, dev[1]), max(n_out)
            aligned = dict(n_units_dev=dev[2], n_out_dev=dev[3])
        audio_res = audio if sample_rate == enc_sr else \
            ctx.resample(audio, int(sample_rate), int(enc_sr), lowpass_filter_width=128, n_dev=n_dev)
        units = self.model(audio_res, rows)
        ratio = (hop_size / sample_rate) / (self.encoder_hop_size / enc_sr)
        return ctx.align_units(units, n_frames, ratio, **aligned)
