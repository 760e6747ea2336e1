"""The splice half of the reference's real-time callback (`gui.py:373-430`) around the device path: sliding input
window bookkeeping is the caller's (PortAudio), the SOLA search + sin^2 cross-fade + tail hand-over run as two
kernels on the stream's own GPU with no host synchronisation.  One `Splicer` per stream (eight
independent streams = eight replicas, no collective), or one `Splicer(rows=S)` for the S streams of a `StreamBank`."""
import numpy as np
import torch

import hipddsp
from controls import EnvelopeMix, KeyTimeline, PitchTune, SpeakerTimeline, UnitIndexBank, check_job_index
from ddsp.analysis import MODEL_FIELDS, _model_field, check_units_width  # noqa: F401  (the two model names stay importable from here)


# ---- the size and key arithmetic of the reference's callback that does not touch audio ------------------------------------
def splice_sizes(samplerate, block_time, crossfade_time, search_time=0.01, delay_time=0.02):
    """(block, xfade, search, delay) in samples at the device rate, truncated as the reference does (`gui.py:319-322`): the
    one place that turns the callback's times into sample counts."""
    return tuple(int(t * samplerate) for t in (block_time, crossfade_time, search_time, delay_time))


def input_frames(samplerate, block_time, crossfade_time, buffer_num, search_time=0.01, delay_time=0.02):
    """Length of the sliding input window at the device rate (`gui.py:323-325`)."""
    block, xfade, search, delay = splice_sizes(samplerate, block_time, crossfade_time, search_time, delay_time)
    return max(block + xfade + search + 2 * delay, (1 + buffer_num) * block)


def hop_size(block_size, samplerate, model_sr):
    """Analysis hop of the window in device samples (`gui.py:94`): a float, non-integral when the device rate differs
    from the model's (557.29 for 512 at 48 kHz over 44.1 kHz)."""
    return block_size * samplerate / model_sr


def window_frames(n_in, hop):
    """Frames of an n_in-sample window at hop `hop` (`Volume_Extractor.extract`, ddsp/vocoder.py:125)."""
    return int(n_in // hop) + 1


def silence_front(block_time, buffer_num, crossfade_time):
    """Seconds of the window's front that the enhancer skips and the f0 extractor may treat as silence
    (`f_safe_prefix_pad_length`, gui.py:326, turned into `silence_front` by gui.py:88-91)."""
    safe = block_time * buffer_num - crossfade_time - 0.01 - 0.02
    return safe - 0.03 if safe > 0.03 else 0


def key_cut_frames(silence, model_sr, block_size):
    """Frames of the f0 track the enhancer drops before it looks at the pitch (`enhancer.py:27-29`)."""
    return int(silence * model_sr / block_size)


def auto_key(f0_max):
    """`adaptive_key='auto'` of `Enhancer.enhance` (enhancer.py:34-38) from the highest f0 of the cut track: the smallest
    non-negative whole number of semitones that brings it to 760 Hz or below (the quotient in fp32, as torch forms it)."""
    with np.errstate(divide="ignore"):
        return int(max(0, np.ceil(12 * np.log2(float(np.float32(f0_max) / np.float32(760))))))


def bank_sizes(samplerate, block_time, crossfade_time, buffer_num, block_size, model_sr, search_time=0.01, delay_time=0.02):
    """The sizes `StreamRenderer` and `StreamBank` work with (gui.py:319-326): a dict of block, xfade, search, delay, n_in
    (samples at the device rate), hop_size (float), frames and silence_front (seconds)."""
    block, xfade, search, delay = splice_sizes(samplerate, block_time, crossfade_time, search_time, delay_time)
    n_in = input_frames(samplerate, block_time, crossfade_time, buffer_num, search_time, delay_time)
    hop = hop_size(block_size, samplerate, model_sr)
    return {"block": block, "xfade": xfade, "search": search, "delay": delay, "n_in": n_in, "hop_size": hop,
            "frames": window_frames(n_in, hop), "silence_front": silence_front(block_time, buffer_num, crossfade_time)}


def output_rate(model_sr, enhancer=None):
    """Rate of what the chain hands to the splice before any resampling: the enhancer's when one is chained
    (`Enhancer.enhance` returns audio at its own rate), otherwise the model's."""
    return int(enhancer.enhancer_sample_rate) if enhancer is not None else int(model_sr)


def phase_vocoder(a, b, fade_out, fade_in):
    """`gui.phase_vocoder` (`gui.py:14-31`) on the device: all four arguments are (n,) device tensors."""
    return hipddsp.context_for(a.device).phase_vocoder(a, b, fade_out, fade_in)


def _check_analysers(name, window, units_encoder, f0_extractor, samplerate, hop, models=()):
    """The analysis front end of `push_audio` as `name` (a class) is given it: both or neither; `f0_extractor` may be the
    shorthand "crepe" or "ac", which `_f0_extractor` builds once every refusal is made.  `models`: the synthesisers the units
    go to, each built for the encoder's channels (`ddsp.analysis.check_units_width`)."""
    if (units_encoder is None) != (f0_extractor is None):
        raise ValueError(f"{name}: push_audio needs both units_encoder and f0_extractor (or neither)")
    if f0_extractor is None:
        return
    shorthand = isinstance(f0_extractor, str) and f0_extractor in ("crepe", "ac")
    if not ((shorthand or hasattr(f0_extractor, "extract")) and hasattr(units_encoder, "encode")):
        raise ValueError(f"{name}: units_encoder / f0_extractor must be ddsp.vocoder.Units_Encoder / F0_Extractor")
    check_units_width(name, units_encoder, *models)
    if not shorthand and (f0_extractor.sample_rate != samplerate or f0_extractor.hop_size != hop):
        raise ValueError(f"{name}: the f0 extractor works at {f0_extractor.sample_rate} Hz with hop "
                         f"{f0_extractor.hop_size}; {window} at {samplerate} Hz with hop {hop}")


def _f0_extractor(f0_extractor, samplerate, hop, f0_min, f0_max, crepe_ckpt, device):
    """gui.py:81-82,93-99: an extractor with these bounds at the device rate and the window's hop, for the shorthands "crepe"
    and "ac" (the autocorrelation extractor: it has no checkpoint and ignores `crepe_ckpt`)."""
    if not isinstance(f0_extractor, str):
        return f0_extractor
    from ddsp.vocoder import F0_Extractor
    return F0_Extractor(f0_extractor, samplerate, hop, float(f0_min), float(f0_max), crepe_ckpt=crepe_ckpt, device=device)


def _check_resample(name, out_sr, samplerate):
    if out_sr != int(samplerate) and hipddsp.load_library().ddsp_resample_length(1, out_sr, int(samplerate)) < 0:
        raise ValueError(f"{name}: cannot resample {out_sr} Hz to {samplerate} Hz")


def _to_device_rate(resamplers, audio, rate, samplerate):
    """`audio` (B, T) at `rate` -> at the device rate; `resamplers` ({(from, to): Resample}) is the caller's cache, filled on
    first use."""
    if rate == int(samplerate):
        return audio
    pair = (int(rate), int(samplerate))
    if pair not in resamplers:
        from resample import Resample
        resamplers[pair] = Resample(pair[0], pair[1], lowpass_filter_width=128)
    return resamplers[pair](audio)


class Splicer:
    def __init__(self, samplerate, block_time, crossfade_time, device, search_time=0.01, delay_time=0.02,
                 use_phase_vocoder=False, rows=None):
        """Sizes as the reference derives them (`gui.py:319-322`).  `rows`: None for one stream, or S for S streams of this
        geometry spliced by one batched call, every row with its own buffer and shift."""
        self.block, self.xfade, self.search, self.delay = splice_sizes(samplerate, block_time, crossfade_time, search_time,
                                                                       delay_time)
        self.device = torch.device(device)
        shape = (self.xfade,) if rows is None else (int(rows), self.xfade)
        self.buffer = torch.zeros(shape, device=self.device)           # `sola_buffer`, gui.py:347
        self.last_shift = None
        # gui.py:349-351 windows, used by the optional phase-vocoder splice (gui.py:417-423); all rows share them
        self.use_phase_vocoder = bool(use_phase_vocoder)
        self.fade_in = torch.sin(torch.pi * torch.arange(0, 1, 1 / self.xfade, device=self.device)[:self.xfade] / 2) ** 2
        self.fade_out = 1 - self.fade_in

    @property
    def ctx(self):
        """The calling thread's context (the audio callback runs on PortAudio's thread, not on the one that built the
        splicer: each thread gets its own scratch arena)."""
        return hipddsp.context_for(self.device)

    def push(self, audio):
        """audio (N,) model output for the current window -> (block,) samples to play (mono; the reference duplicates them
        to two channels on the host, `gui.py:430`); with `rows`, (rows, N) -> (rows, block)."""
        kept = self.buffer.clone() if self.use_phase_vocoder else None
        emitted, shift = self.ctx.sola(audio, self.buffer, self.block, self.xfade, self.search, self.delay)
        self.last_shift = shift
        if self.use_phase_vocoder:
            # every row's head at its own SOLA shift (the shifts stay on the device: a gather, no host sync)
            n = audio.shape[-1]
            start = n - self.block - self.xfade - self.search - self.delay
            idx = start + shift.to(torch.int64)[:, None] + torch.arange(self.xfade, device=self.device)[None, :]
            head = audio.reshape(-1, n).gather(1, idx).reshape(kept.shape)
            emitted[..., :self.xfade] = self.ctx.phase_vocoder(kept, head, self.fade_out, self.fade_in)
        return emitted


class StreamRenderer:
    """One real-time stream on one GPU: the device half of the reference's callback chain
    (`gui.GUI.audio_callback`, gui.py:367-433, calling `gui.SvcDDSP.infer`, gui.py:69-140).

    Per block of `block` input samples at the device rate `samplerate`:
      1. the sliding input window takes the block (`input_wav[:] = append(input_wav[block:], indata)`, gui.py:373-374);
      2. frame volume of the window at hop `hop_size = block_size * samplerate / model_sr` (`Volume_Extractor.extract`,
         gui.py:94,105-106) -> `ddsp_volume_extract`, or `ddsp_volume_extract_frac` when that hop is not integral;
      3. f0 and units of the window (gui.py:94-102,114-116).  `push_audio` computes them on the device with this package's
         `F0_Extractor('crepe')` (uv_interp, the silent front, bounds `f0_min` / `f0_max`, both at the device rate and the
         window's hop) and `Units_Encoder('hubertsoft')`, given as `f0_extractor=` / `units_encoder=`; `push_block` takes them
         from the caller instead (`units=`, `f0=`, or a `features(window) -> (units (1,Fr,C), f0 (1,Fr,1))` callable: other
         extractors and encoders).  f0 is shifted by `pitch_adjust` semitones (gui.py:102);
      4. the synthesiser forward (gui.py:125-126) with `spk_id` or `spk_mix_dict`, eager or replayed from a HIP graph
         captured for the current mix: `graphed.GraphedSynth` under `push_block`; under `push_audio` steps 1-5 are ONE graph
         (`graphed.GraphedBlock` over the one window), replayed with one host call per block;
      5. `output *= mask` with the 9-frame dilated volume gate at the model's `block_size` (gui.py:107-112,127) ->
         `ddsp_volume_gate`, in place;
      6. optionally `enhancer.enhance(...)` (gui.py:128-134), eager, with the adaptive key decided here (see below);
      7. resampling from the model's (or enhancer's) rate to `samplerate` when they differ (gui.py:399-404);
      8. SOLA search + cross-fade + tail hand-over (gui.py:405-430) -> `Splicer.push`.
    Without the enhancer nothing in the chain synchronises with the host, the analysis included; the returned (block,) tensor
    is what the callback copies out.  After a `push_audio`, `last_f0` (1, Fr, 1) (shifted), `last_units` (1, Fr, C) and
    `last_volume` (1, Fr) hold the window's analysis (under the graph: static tensors, valid until the next block).  With `enhancer_adaptive_key='auto'` the key (it decides tensor lengths) is taken before the synthesis is
    enqueued: on the host when f0 arrives as a CPU tensor, else by one scalar read-back of the f0 maximum.
    Streams are independent.  One renderer is one stream; several streams of one geometry on one GPU are a `StreamBank`
    (one graph replay per block for all of them), and across GPUs they are replicas."""

    def __init__(self, model, samplerate, block_time, crossfade_time, device, buffer_num=4, threshold_db=-45.0, spk_id=1,
                 features=None, use_graph=True, use_phase_vocoder=False, pitch_adjust=0, spk_mix_dict=None, enhancer=None,
                 enhancer_adaptive_key="auto", units_encoder=None, f0_extractor=None, f0_min=50, f0_max=1100, f0_dither=True,
                 crepe_ckpt=None):
        self.model = model.eval()
        self.device = torch.device(device)
        self.block_size = int(model.block_size)
        self.model_sr = int(model.sampling_rate)
        self.samplerate = samplerate
        self.hop = self.block_size                                   # the model's hop: gate, synthesis
        self.threshold_db = float(threshold_db)
        self.pitch_adjust = float(pitch_adjust)
        self.splicer = Splicer(samplerate, block_time, crossfade_time, self.device, use_phase_vocoder=use_phase_vocoder)
        z = bank_sizes(samplerate, block_time, crossfade_time, buffer_num, self.block_size, self.model_sr)
        self.block, self.n_in, self.silence_front = z["block"], z["n_in"], z["silence_front"]
        self.hop_size, self.frames = z["hop_size"], z["frames"]    # the window's analysis hop; frames of f0 / units / volume alike
        self.window = torch.zeros(self.n_in, device=self.device)   # `self.input_wav`, gui.py:346
        if isinstance(enhancer_adaptive_key, str) and enhancer_adaptive_key != "auto":
            raise ValueError(f"enhancer_adaptive_key must be a number or 'auto', got {enhancer_adaptive_key!r}")
        self.enhancer = enhancer
        self.enhancer_adaptive_key = enhancer_adaptive_key
        self.last_key = None                                         # the key the last block was enhanced with
        self.out_sr = output_rate(self.model_sr, enhancer)
        _check_resample("StreamRenderer", self.out_sr, samplerate)
        self._resamplers = {}
        self.spk_id = torch.full((1, 1), int(spk_id), dtype=torch.int64, device=self.device)
        self.spk_mix_dict = self._checked_mix(spk_mix_dict)
        self.features = features
        _check_analysers("StreamRenderer", "this renderer's window is", units_encoder, f0_extractor, samplerate, self.hop_size,
                         (self.model,))
        f0_extractor = _f0_extractor(f0_extractor, samplerate, self.hop_size, f0_min, f0_max, crepe_ckpt, self.device)
        self.units_encoder, self.f0_extractor, self.f0_dither = units_encoder, f0_extractor, bool(f0_dither)
        self.last_f0 = self.last_units = self.last_volume = None
        self.use_graph = bool(use_graph)
        self.graph = None                                            # the synthesis graph of `push_block`
        self.block_graph = None                                      # the whole-block graph of `push_audio`
        self.graph_builds = 0                                        # captures so far (a mix change re-captures)
        if self.use_graph:
            self._capture()

    def _capture(self):
        """(Re-)captures for the current mix: the whole-block graph when the analysis is configured (the synthesis-only graph
        of `push_block(units=, f0=)` is then captured on its first use), else the synthesis graph."""
        import graphed
        self.graph = self.block_graph = None                         # the old captures are released before the new one
        if self.f0_extractor is not None:
            self.block_graph = graphed.GraphedBlock(
                self.model, self.units_encoder, self.f0_extractor, self.window, self.block, self.samplerate, self.hop_size,
                self.silence_front, self._pitch_factor(), self.threshold_db, spk_mix_dict=self.spk_mix_dict,
                f0_dither=self.f0_dither)
        else:
            self.graph = graphed.GraphedSynth(self.model, 1, self.frames, spk_mix_dict=self.spk_mix_dict)
        self.graph_builds += 1

    def _pitch_factor(self):
        return 2 ** (self.pitch_adjust / 12) if self.pitch_adjust != 0 else 1

    def _checked_mix(self, spk_mix_dict):
        if spk_mix_dict is None:
            return None
        n_spk = int(self.model.unit2ctrl.n_spk)
        mix = {int(k): float(v) for k, v in spk_mix_dict.items()}
        if not 1 <= len(mix) <= 16 or any(not 1 <= k <= n_spk for k in mix):
            raise ValueError(f"StreamRenderer: a speaker mix holds 1 to 16 ids in [1, {n_spk}], got {spk_mix_dict}")
        return mix

    def set_speaker(self, spk_id=None, spk_mix_dict=None):
        """Live speaker change (the GUI's speaker id / "set mix"): `spk_mix_dict` replaces the mix (None = use `spk_id`),
        `spk_id` (if given) replaces the id.  A new mix re-captures the graph (its weights are kernel arguments); an id
        alone does not (it is a static input of the capture)."""
        n_spk = int(self.model.unit2ctrl.n_spk)
        if spk_id is not None and not 1 <= int(spk_id) <= n_spk:
            raise ValueError(f"StreamRenderer: spk_id must be in [1, {n_spk}], got {spk_id}")
        mix = self._checked_mix(spk_mix_dict)
        if spk_id is not None:
            self.spk_id.fill_(int(spk_id))
        if mix != self.spk_mix_dict:
            self.spk_mix_dict = mix
            if self.use_graph:
                self._capture()

    def _key(self, f0):
        """The enhancer's key for this window: a number as configured, or the reference's 'auto' rule over the track
        after the enhancer's front cut (host arithmetic on a CPU track, one scalar read-back otherwise)."""
        if not isinstance(self.enhancer_adaptive_key, str):
            return self.enhancer_adaptive_key
        cut = key_cut_frames(self.silence_front, self.model_sr, self.block_size)
        return auto_key(float(torch.max(f0[:, cut:])))

    @torch.no_grad()
    def push_block(self, block_in, units=None, f0=None, noise=None, rand_ini=None):
        """block_in (block,) device samples of the stream -> (block,) samples to play.  `units` (1, Fr, C) and `f0`
        (1, Fr, 1) of the CURRENT window may be passed instead of a `features` callable; `noise` (1, Fr*hop) in [0, 1)
        replaces the fresh draw and `rand_ini` (9,) the enhancer's source phases (parity tests)."""
        if block_in.numel() != self.block:
            raise ValueError(f"StreamRenderer: a block is {self.block} samples, got {block_in.numel()}")
        if (units is None or f0 is None) and self.features is None and self.f0_extractor is not None:
            return self.push_audio(block_in, noise=noise, rand_ini=rand_ini)
        ctx = hipddsp.context_for(self.device)
        if self.f0_extractor is None:
            self.window = torch.cat([self.window[self.block:], block_in.reshape(-1).to(self.device, torch.float32)])
        else:   # a whole-block graph may hold the window's address: the same shift, in place
            ctx.stream_push_(self.window, block_in.reshape(-1).to(self.device, torch.float32).contiguous())
        if units is None or f0 is None:
            if self.features is None:
                raise ValueError("StreamRenderer: pass units and f0, or construct it with a `features` callable")
            units, f0 = self.features(self.window)
        if units.shape[1] != self.frames or f0.shape[1] != self.frames:
            raise ValueError(f"StreamRenderer: the window has {self.frames} frames")
        if self.pitch_adjust != 0:
            f0 = f0 * 2 ** (self.pitch_adjust / 12)
        key = None
        if self.enhancer is not None:
            key = self._key(f0)                                      # before anything of this block is enqueued
        units, f0 = units.to(self.device), f0.to(self.device)
        volume = ctx.volume_extract(self.window[None], self.hop_size)   # (1, Fr)
        if volume.shape[1] != self.frames:
            raise ValueError(f"StreamRenderer: the window has {self.frames} frames")
        if self.use_graph and self.graph is None:                    # (a renderer whose captures so far were whole blocks)
            import graphed
            self.graph = graphed.GraphedSynth(self.model, 1, self.frames, spk_mix_dict=self.spk_mix_dict)
            self.graph_builds += 1
        if self.graph is not None:
            sig = self.graph(units, f0, volume, self.spk_id, noise=noise)[0]
        elif noise is not None:
            sig = self.model(units, f0, volume, self.spk_id, spk_mix_dict=self.spk_mix_dict, noise=noise)[0]
        else:
            sig = self.model(units, f0, volume, self.spk_id, spk_mix_dict=self.spk_mix_dict)[0]
        ctx.volume_gate_(sig, volume, self.threshold_db, self.hop)
        rate = self.model_sr
        if self.enhancer is not None:
            sig, rate = self.enhancer.enhance(sig, self.model_sr, f0, self.block_size, adaptive_key=key,
                                              silence_front=self.silence_front, rand_ini=rand_ini)
            self.last_key = key
        return self.splicer.push(_to_device_rate(self._resamplers, sig, rate, self.samplerate)[0])

    @torch.no_grad()
    def push_audio(self, block_in, noise=None, rand_ini=None):
        """block_in (block,) raw samples of the stream at the device rate -> (block,) samples to play: the whole of
        gui.py:373-430, the analysis included (class docstring, steps 1-8).  With `use_graph` steps 1-5 are one graph replay,
        else the same calls run eagerly; `noise` and `rand_ini` as in `push_block`."""
        if self.f0_extractor is None:
            raise ValueError("StreamRenderer: push_audio needs units_encoder= and f0_extractor= at construction")
        if block_in.numel() != self.block:
            raise ValueError(f"StreamRenderer: a block is {self.block} samples, got {block_in.numel()}")
        block_in = block_in.reshape(-1).to(self.device, torch.float32).contiguous()
        if self.block_graph is not None:
            sig, f0, units, volume = self.block_graph(block_in, self.spk_id, noise=noise)
        else:
            import graphed
            sig, f0, units, volume = graphed.block_chain(
                hipddsp.context_for(self.device), self.model, self.units_encoder, self.f0_extractor, self.window, block_in,
                self.samplerate, self.hop_size, self.silence_front, self._pitch_factor(), self.threshold_db, self.hop,
                {"spk_id": self.spk_id, "spk_mix_dict": self.spk_mix_dict}, noise, self.f0_dither)
        self.last_f0, self.last_units, self.last_volume = f0, units, volume
        rate = self.model_sr
        if self.enhancer is not None:
            key = self._key(f0)                                      # (one scalar read-back under 'auto': it decides lengths)
            sig, rate = self.enhancer.enhance(sig, self.model_sr, f0, self.block_size, adaptive_key=key,
                                              silence_front=self.silence_front, rand_ini=rand_ini)
            self.last_key = key
        return self.splicer.push(_to_device_rate(self._resamplers, sig, rate, self.samplerate)[0])


def active_width(A, widths):
    """The batch width at which a `StreamBank` call with A active slots runs: the smallest W >= A of the bank's ladder `widths`
    (sorted).  Rows A..W-1 of the compact batch are padding.  ValueError when no width holds A rows."""
    if isinstance(A, bool) or not isinstance(A, int) or A < 1:
        raise ValueError(f"active_width: a call names at least one slot, got {A!r}")
    for W in widths:
        if W >= A:
            return int(W)
    raise ValueError(f"active_width: {A} active slots, the widest batch of the ladder {tuple(widths)} holds {max(widths, default=0)}")


def _check_active_widths(active_widths, S, name="active_widths"):
    """`StreamBank(active_widths=)` (or `model_widths=`, as `name`) -> the ladder: the sorted distinct ints in 1..S as given, with S
    behind them if missing."""
    widths = tuple(active_widths) if isinstance(active_widths, (tuple, list)) else None
    if widths is None or any(isinstance(w, bool) or not isinstance(w, int) or not 1 <= w <= S for w in widths) or \
            any(a >= b for a, b in zip(widths, widths[1:])):
        raise ValueError(f"StreamBank: {name} must be a sorted tuple of distinct ints in 1..{S}, got {active_widths!r}")
    return widths if widths and widths[-1] == S else widths + (S,)


def default_model_widths(S):
    """The ladder of `StreamBank(models=...)` when `model_widths` is not given: the powers of two up to S, and S."""
    return tuple(w for w in (1 << i for i in range(int(S).bit_length())) if w < S) + (int(S),)


MAX_GLIDE_POINTS = 64             # breakpoints of one slot's speaker timeline (`ddsp_bank_glide`'s P_max)


def _check_models(model, models):
    """`StreamBank(model, ..., models=)` -> the list of models: host comparisons only.  The models of a bank share the analysis, the
    enhancer stage and the splice, so they agree in `MODEL_FIELDS`; class, weights, `n_spk` and `c` are each model's own."""
    if models is None:
        return [model]
    models = list(models) if isinstance(models, (tuple, list)) else []
    if not models:
        raise ValueError("StreamBank: models must be a non-empty list of synthesisers")
    if model is not None and model is not models[0]:
        raise ValueError("StreamBank: with models= the positional model is None or models[0] itself (it names model 0)")
    for k, m in enumerate(models[1:], 1):
        for field in MODEL_FIELDS:
            a, b = _model_field(models[0], field), _model_field(m, field)
            if a != b:
                raise ValueError(f"StreamBank: models[{k}].{field} is {b}, models[0].{field} is {a}: the models of a bank agree in "
                                 f"{', '.join(MODEL_FIELDS)}")
    return models


class _Rows:
    """What the chain of a `StreamBank` runs on at one batch width W: `windows` (W, n_in), the `splicer` with its (W, xfade)
    buffer, the tables `spk_ids` / `spk_w` (W, K), `pitch` (W,) and `request` (W,) (the enhancer's key requests, or None), and
    under `use_graph` the captures over them.  The bank's own state is the width-S instance; its window push is
    `ddsp_stream_push`.  A compact instance (`active_widths`) has tensors of its own and a device row table `rows` (W,) int32,
    entry r the slot of row r or -1 for padding, all padding until a call names its slots: its push is `ddsp_bank_gather` from the
    bank's state, and `scatter` (`ddsp_bank_scatter`) brings the spliced buffers back to the slots.  On a bank with
    `glide_breakpoints` every instance has a static `w_frames` (W, Fr, K) too: its push ends with `ddsp_bank_glide`, which fills
    it from the SLOTS' glide state through the row table, and `mix` - what the synthesis takes as its speaker term - is then the
    per-frame pair (`spk_ids`, `w_frames`) instead of the row pair (`spk_ids`, `spk_w`)."""

    def __init__(self, bank, W, compact):
        self.bank, self.W, self.A = bank, int(W), int(W)
        self.graph = self.bank_graph = self.enhancer_graph = None
        self.rows = self.request = self.w_frames = self.pitch_frames = None
        if bank.pitch_breakpoints is not None:
            self.pitch_frames = torch.ones(self.W, bank.frames, device=bank.device)
        if bank.glide_breakpoints is not None:
            self.w_frames = torch.zeros(self.W, bank.frames, bank.max_mix, device=bank.device)
            self.w_frames[:, :, 0] = 1.0
        if not compact:
            self.windows, self.splicer, self.spk_ids, self.spk_w, self.pitch = bank.windows, bank.splicer, bank.spk_ids, bank.spk_w, bank.pitch
            if bank.enhancer is not None:
                self.request = bank.enhancer_request
            return
        dev = bank.device
        self.rows = torch.full((self.W,), -1, dtype=torch.int32, device=dev)
        self.windows = torch.zeros(self.W, bank.n_in, device=dev)
        self.splicer = Splicer(*bank._splicer_args, rows=self.W)
        self.spk_ids = torch.ones(self.W, bank.max_mix, dtype=torch.int32, device=dev)
        self.spk_w = torch.zeros(self.W, bank.max_mix, device=dev)
        self.spk_w[:, 0] = 1.0
        self.pitch = torch.ones(self.W, device=dev)
        if bank.enhancer is not None:
            self.request = torch.zeros(self.W, dtype=torch.int32, device=dev)

    def select(self, active):
        """The slots of this call: one small upload into the row table, whose address the captured kernels hold."""
        if self.rows is not None:
            self.A = len(active)
            self.rows.copy_(torch.tensor(list(active) + [-1] * (self.W - self.A), dtype=torch.int32))

    @property
    def mix(self):
        """The speaker term of this instance's synthesis (`spk_mix_rows=`): a mix per row, or per frame on a bank that glides."""
        return self.spk_ids, (self.spk_w if self.w_frames is None else self.w_frames)

    @property
    def formant_term(self):
        """The formant term of this instance's synthesis (`forward_formant`'s `formant`): None on a bank without `formant`; the
        slots' row of factors at the full width; with the width's row table behind it on a compact instance, so a row reads
        its SLOT's factor and a padding row none."""
        f = self.bank.formant
        return None if f is None else (f if self.rows is None else (f, self.rows))

    @property
    def tune_term(self):
        """The pitch-correction term of this instance's chain (`graphed.block_chain`'s `tune`): None on a bank without `tune`;
        the slots' settings, with the width's row table as the owner of every row on a compact instance (a padding row has none)."""
        b = self.bank
        return None if b.tune_mask is None else (b.tune_mask, b.tune_param, self.rows)

    @property
    def retrieve_term(self):
        """The unit-retrieval term of this instance's chain (`graphed.block_chain`'s `retrieve`): None on a bank without
        `indices`; the bank of indices and the slots' rows, with the width's row table as the owner of every row on a compact
        instance (a padding row has none)."""
        b = self.bank
        return None if b.indices is None else (b.indices, b.index_of_slot, b.ratio_of_slot, b.retrieve_k, self.rows)

    @property
    def envelope_term(self):
        """The envelope-mix term of this instance's chain (`graphed.block_chain`'s `envelope`): None on a bank without
        `envelope`; the slots' rates, the two hops and the window, with the width's row table as the owner of every row on a
        compact instance (a padding row has none)."""
        b = self.bank
        return None if b.rate_of_slot is None else (b.rate_of_slot, *b.envelope_setting, self.rows)

    @property
    def pitch_term(self):
        """The pitch term of this instance's chain: a factor per row, or per frame on a bank with `pitch_breakpoints`."""
        return self.pitch if self.pitch_frames is None else self.pitch_frames

    def push(self, ctx, windows, blocks):
        """`graphed.block_chain`'s push step: `windows` (this instance's) come up to date with `blocks` (W, block); on a bank
        with `glide_breakpoints` the weights of the block's frames follow, and the clocks of the call's slots advance; on one
        with `pitch_breakpoints` the f0 factors of the block's frames and the key clocks likewise."""
        b = self.bank
        if self.rows is None:
            ctx.stream_push_(windows, blocks)
        else:
            ctx.bank_gather_(self.rows, blocks, b.windows, windows, b.sola_buffer, self.splicer.buffer, (b.spk_ids, b.spk_w),
                             (self.spk_ids, self.spk_w), b.pitch, self.pitch, None if self.request is None else b.enhancer_request,
                             self.request)
        if self.w_frames is not None:
            ctx.bank_glide_(self.rows, b.glide_clock, b.glide_n, b.glide_t, b.glide_w, b.spk_w, self.w_frames, b.n_in, b.block,
                            b.hop_size)
        if self.pitch_frames is not None:
            ctx.bank_key_glide_(self.rows, b.key_clock, b.key_n, b.key_t, b.key_semi, b.key_fac, b.pitch, self.pitch_frames, b.n_in,
                                b.block, b.hop_size)
        return windows

    def scatter(self):
        if self.rows is not None:
            hipddsp.context_for(self.bank.device).bank_scatter_(self.rows, self.splicer.buffer, self.bank.sola_buffer)

    def pad(self, t, fill=0.0):
        """Per-row input (A, ...) -> (W, ...): the padding rows behind the real ones."""
        if t.shape[0] == self.W:
            return t
        return torch.cat([t, t.new_full((self.W - t.shape[0], *t.shape[1:]), fill)])

    def real(self, *ts):
        """Per-row results (W, ...) -> the A real rows of each."""
        return ts if self.A == self.W else tuple(t[:self.A] for t in ts)


class StreamBank:
    """S real-time streams of ONE geometry (device rate, block, cross-fade, window) on one GPU, all advanced by one block per
    call: the chain of `StreamRenderer` (its docstring, steps 1-8) with every step batched over the streams.  Under
    `push_audio` steps 1-5 of all rows are ONE linear HIP-graph replay (`graphed.GraphedBlock` over the S windows); then come
    resampling to the device rate and the batched splice (a `Splicer(rows=S)` -> `ddsp_sola` with S rows: every row's own arg-max,
    buffer and tail).

    With `enhancer=` (an `enhancer.Enhancer`) step 6 runs on all rows too, every row with an adaptive key of its own
    (`Enhancer.enhance_keyed`): the key - the reference's 'auto' rule, or what `set_enhancer_key` fixed for the slot - is decided
    on the device from the shifted f0, and it picks the row's working rate inside the kernels, so nothing is read back and
    a pitch that crosses a key boundary captures nothing anew.  The result is resampled to the device rate on the device
    lengths and every row's last block + xfade + search + delay samples, counted from the row's OWN end (`gui.py:405-406`), go to
    the splice.  Under `use_graph` the stage is a second graph (`graphed.GraphedBankEnhancer`) replayed right after the first;
    `graph_builds` stays 1.  `last_key` (S,) int32 holds the keys of the block and `last_signal` the (S, block + xfade + search +
    delay) tails.  DIVERGENCE: keys are clamped to `enhancer_max_key` (0..12, default 12 = one octave); the reference's key is
    unbounded, a bank needs a finite set of working rates.

    State, all on the device: `windows` (S, n_in), `sola_buffer` (S, xfade), the speaker mix of every slot `spk_ids` (S, K)
    int32 / `spk_w` (S, K) fp32 with K = `max_mix`, and `pitch` (S,), a factor.  The captured kernels read the three per-slot
    tables when they run: `set_speaker`, `set_pitch` and `reset` write device rows only, and `graph_builds` stays at 1 for
    the life of the bank.  A bank is built for one of two forms: with `units_encoder` / `f0_extractor` it takes raw audio
    (`push_audio`); without them it takes the caller's units and f0 (`push_block`, over a `graphed.GraphedSynth` with row
    mixes).

    After a call `last_f0` (S, Fr, 1) (shifted), `last_units` (S, Fr, C), `last_volume` (S, Fr), `last_shift` (S,) int32 and
    `last_signal` (S, N), the gated and resampled signal the splice consumed, hold that block's values (under the graph:
    static tensors, valid until the next block).

    Active sets (`active_widths=`, a sorted tuple of distinct ints in 1..S; S is appended if missing; None: the feature is off
    and nothing of it is allocated or captured).  A push call with `active=`, a strictly increasing sequence of A slot ints,
    advances only those slots: its per-row arguments (`blocks` (A, block), `units`, `f0`, `noise`, a 2-D `rand_ini`), its result
    and every `last_*` tensor have A rows, row r belonging to slot active[r], and `last_active` holds the slots.  The A rows run as
    a compact batch of width W = `active_width(A, active_widths)`, the smallest width of the ladder that holds them: the same
    chain on tensors of that width (`_Rows`), with `ddsp_bank_gather` as the window push - it pushes the blocks into the named
    slots' own windows and copies their windows, SOLA buffers, mixes, pitches and key requests to the compact rows - and
    `ddsp_bank_scatter` after the splice, which returns the spliced buffers.  Both read a device row table (W,) int32 that one
    small upload rewrites before the call, so under `use_graph` every width is captured once, at construction: `graph_builds` is
    1 + len(active_widths) (the appended S counted) for the life of the bank, the chain and the enhancer stage of a width
    counting as one build as they do for the full width.  Rows A..W-1 are padding: a zero window, speaker 1 with weight 1, pitch 1
    and key request 0; they are computed, never written back to a slot and never returned.
    PAUSED SLOTS: a slot that a call does not name keeps its rows of `windows`, `sola_buffer`, `spk_ids`, `spk_w`, `pitch` and
    `enhancer_request` (and of the glide state, below) bit for bit, and a caller that is named again carries on where it stopped; `reset(slot)` remains the way
    to hand a slot to someone new.  A call without `active` is the full-width call on its own graph, on a bank with
    `active_widths` too: there an idle slot is a slot that is fed zeros; its rows are computed like every other row, and its
    output is zero through the volume gate.  Every refusal of a call (`active` on a bank without `active_widths`, an empty,
    unsorted or repeated `active`, a slot outside [0, S), a bool or non-int slot, per-row arguments that do not have A rows) is a
    ValueError raised before anything is uploaded or launched.

    A model per slot (`models=[m0, m1, ...]`; without it nothing of this is allocated or captured, and `StreamBank(model)` is the
    bank above, bit for bit).  The positional `model` is then None or `models[0]` itself: it names model 0, anything else is
    refused.  The models may differ in class (CombSub, Sins, CombSubFast), weights, `n_spk` and `c`; they agree in
    `sampling_rate`, `block_size` and unit width and sit on one device (ValueError naming the model and the field, before any
    device call).  `set_model(slot, k, spk_id=1, spk_mix_dict=None)` gives a slot its model (`model_of_slot`, host state) and a
    speaker valid for it; `set_speaker` checks ids against the slot's own model's `n_spk`; `reset` keeps the model.  Per call the
    window push and the analysis (volume, f0, units) run ONCE over the call's rows - the full width, or the compact width of
    `active=` - as the same chain stopped after the features (`graphed.block_chain(model=None)`).  Then every model that owns a
    row of the call renders its rows as a compact batch (`graphed.GraphedModelRows`, one per model and width of `model_widths`:
    a sorted tuple of distinct ints in 1..S, S appended if missing; default the powers of two up to S, and S):
    `ddsp_bank_features_gather` by a device row table over the call's rows, the model's forward with mix rows, the gate, and
    `ddsp_bank_signal_scatter` into the call's (rows, T) signal; the smallest width that holds the model's rows is replayed, a
    model without rows is not.  Padding rows of such a batch compute on zero units, f0 0, volume 0 and speaker 1, and are never
    scattered.  Enhancer stage (one generator for all models), resampling and splice follow over all rows as above.  Every chain
    is captured at construction: `graph_builds` is the count above plus len(models) * len(model_widths), and a change of
    assignment captures nothing.  The paused-slot rule holds as it stands.

    A voice that glides (`glide_breakpoints=P_max`, an int in 1..64; None: nothing of this is allocated, captured or launched,
    and the bank is the bank above, bit for bit).  Every slot then has a clock and a speaker timeline on the device:
    `glide_clock` (S,) int64, the device samples pushed into the slot since its timeline started; `glide_n` (S,) int32, its
    breakpoint count, 0 = none; `glide_t` (S, P_max) int64, the breakpoint times in device samples; `glide_w` (S, P_max, K) their
    weights.  `set_timeline(slot, timeline, at=0.0)` writes them from an `infer_offline.SpeakerTimeline`, time 0 being the first
    sample pushed after the call.  Every push ends with one launch of `ddsp_bank_glide` over the call's rows: frame t of a window
    has stream time clock + block - n_in + t * hop_size, its weights are the timeline interpolated there (the slot's `spk_w` row
    where it has none, the padding speaker on a padding row), and the clocks of the call's slots advance by one block.  The
    synthesis of every chain takes the per-frame pair (`spk_ids`, those weights) where it took (`spk_ids`, `spk_w`); a constant
    mix renders to the same bits either way.  Under `push_audio` the launch is part of the captured block, so a glide is device
    data like everything else: `graph_builds` is what it was, and setting, clearing or running a timeline captures nothing.
    `set_speaker` ends a slot's glide, `reset` restarts its clock and keeps its timeline, `last_mix_w` (A, Fr, K) holds the
    block's weights.  The paused-slot rule covers `glide_clock`, `glide_n`, `glide_t` and `glide_w`: a paused slot's voice stands
    still and goes on from there when the slot is named again.  Refused: `glide_breakpoints` with `models=`; `set_timeline` on
    a bank without `glide_breakpoints`, with more points than it, two points on one sample, more ids than `max_mix` or an id
    outside the slot's model.

    A key that glides (`pitch_breakpoints=P_max`, an int in 1..64; None: nothing of this is allocated, captured or launched, and
    the bank is the bank above, bit for bit).  Independent of `glide_breakpoints`, and allowed with `models=`, `active_widths=`
    and the enhancer: the pitch is applied to f0 in the shared analysis of a block, in front of every per-model row gather.
    Every slot then has `key_clock` (S,) int64, `key_n` (S,) int32 (0 = no timeline), `key_t` (S, P_max) int64 in device samples
    and `key_semi` / `key_fac` (S, P_max) fp32, the breakpoints' semitones and their factors 2 ** (key / 12) formed on the host
    as `set_pitch` forms its one.  `set_pitch_timeline(slot, infer_offline.KeyTimeline, at=0.0)` writes them.  Every push ends
    with one launch of `ddsp_bank_key_glide` over the call's rows (beside `ddsp_bank_glide` when both are on): frame t of a
    window has stream time key_clock + block - n_in + t * hop_size and gets the timeline's factor there - linear in semitones
    between two points, a point's stored factor at and outside the points and on constant stretches, so a constant timeline
    emits the bits of `set_pitch` -, the slot's `pitch` where it has no timeline and 1 on a padding row; the key clocks of the
    call's slots advance by one block.  The chain multiplies f0 with these per-frame factors (`_Rows.pitch_frames` (W, Fr))
    where it multiplied with `pitch`.  Part of the captured block under `push_audio`: `graph_builds` is what it was, and
    setting, ending (`set_pitch`) or restarting (`reset`) a timeline captures nothing.  `last_pitch` (A, Fr) holds the block's
    factors.  The paused-slot rule covers `key_clock`, `key_n`, `key_t`, `key_semi` and `key_fac`.  Refused:
    `set_pitch_timeline` on a bank without `pitch_breakpoints`, with more points than it, or two points on one sample.

    A formant shift per slot (`formant=True`; the default False allocates, captures and launches nothing of this, and the bank
    is the bank above, bit for bit).  Every slot then has a row of `formant` (S,) fp32, a FACTOR, initially 1;
    `set_formant(slot, semitones)` writes 2 ** (semitones / 12) there (|semitones| <= 24) and `reset(slot)` puts 1 back: device
    rows only, `graph_builds` stays what it was.  Every chain of such a bank enters the synthesiser through `forward_formant` with
    the slots' row - at a compact width with the width's row table behind it, so a row reads its slot's factor and a padding
    row none -: one `ddsp_ctrl_warp` launch between the control network and the filter synthesis, inside the captured block.  The
    kernels only read the row, so a paused slot's factor stays as it is.  Works with `glide_breakpoints`, `pitch_breakpoints`,
    `active_widths` and the enhancer (which is not told of the shift: it follows f0).  Refused: `formant=True` with `models=`;
    `set_formant` on a bank without it.

    Pitch correction per slot (`tune=True`; the default False allocates, captures and launches nothing of this, and the bank is
    the bank above, bit for bit).  Every slot then has a row of `tune_mask` (S,) int32 and `tune_param` (S, 3) fp64 (a4, strength,
    alpha), initially off (mask 0); `set_tune(slot, PitchTune | None)` writes the slot's setting with
    hop_seconds = hop_size / samplerate and `reset(slot)` switches it off: device rows only, `graph_builds` stays what it was.
    Every chain of such a bank runs one `ddsp_f0_tune` launch right behind the pitch multiply (include/ddsp_amd.h states the
    rule) - inside the captured block under `push_audio`, behind the multiply of `push_block` -, at a compact width with the
    width's row table as the owner of every row.  It sits in the shared analysis, so it works with `models=` as well as with
    `active_widths`, `pitch_breakpoints`, `glide_breakpoints`, `formant` and the enhancer, which sees the corrected f0.
    DIVERGENCE: the correction's recurrence restarts at the first frame of the re-rendered window in every block; the window
    is at least a second long, only its tail is spliced and the cross-fade hides the rest.  The bank carries no state for it,
    so a paused slot has none to keep.  Refused: `set_tune` on a bank without it.

    Unit retrieval per slot (`indices=UnitIndexBank`, `retrieve_k`; the default None allocates, captures and launches nothing
    of this, and the bank is the bank above, bit for bit).  Every slot then has a row of `index_of_slot` (S,) int32, -1 at first,
    and `ratio_of_slot` (S,) fp32; `set_index(slot, i | None, ratio=0.5)` writes them and `reset(slot)` switches the slot off:
    device rows only, `graph_builds` stays what it was.  Every `push_audio` chain of such a bank runs `ddsp_units_retrieve` (two
    launches; include/ddsp_amd.h states the rule) right behind `units_encoder.encode` - inside the captured block, and on the
    eager path alike -, at a compact width with the width's row table as the owner of every row.  The kernels only read the
    slots' rows, so a paused slot keeps everything.  It sits in the shared analysis, in front of the per-model row gather, so it
    works with `models=` as well as with `active_widths` and the enhancer.  The bank's workspace is reserved here, before any
    capture, for S rows of the window's frames: `ddsp_units_retrieve_workspace` grows with the rows, so that size serves every
    narrower width of the ladder.  The `UnitIndexBank`'s one workspace serves one stream at a time: banks that push on different
    streams take a `UnitIndexBank` each.  Refused: `set_index` on a bank without indices; an index number outside the bank;
    a bank of indices on another device or of another unit width than the encoder's.  `push_block` takes the caller's units
    as they are.

    Envelope mix per slot (`envelope=True`, `envelope_hop_seconds`, `envelope_frames`; the default False allocates, captures and
    launches nothing of this, and the bank is the bank above, bit for bit).  RVC's `rms_mix_rate` in its real-time form: the
    rendered signal is held to the loudness envelope of the slot's INPUT window (include/ddsp_amd.h states the rule at
    `ddsp_envelope_rms`), frames `envelope_hop_seconds` apart (RVC: 10 ms) with a window of `envelope_frames` hops (RVC: 4).
    Every slot has a row of `rate_of_slot` (S,) fp64, 1 at first, which is off; `set_envelope(slot, rate | None)` writes it
    and `reset(slot)` switches the slot off: a device row only, `graph_builds` stays what it was.  Every `push_audio` chain of
    such a bank runs three calls right behind the gate - the frame RMS of the windows at the device rate, the frame RMS of the
    gated signal at the model's rate, the apply in place - inside the captured block and on the eager path alike, at a compact
    width with the width's row table as the owner of every row.  A slot whose rate is 1 is selected around: with every slot off
    the bank emits the bits of a bank without the feature.  The kernels only read the slots' rows, so a paused slot keeps its
    rate.  It works with `active_widths`, `tune`, `indices`, the glides, `formant` and the enhancer.  DIVERGENCE: the enhancer
    stage FOLLOWS the matched signal (RVC and the offline jobs match the final output); a silent input window silences the
    slot, as in RVC.  Refused: `envelope=True` with `models=` (the signal is rendered per model, behind the block), or on a bank
    without analysers (`push_block`); `set_envelope` on a bank without it.

    Not in the bank: an envelope mix on a bank with `models=`; a formant shift on a bank with `models=`, or one that moves along a timeline; streams of different geometry; models of different sampling rate, block size or unit width; a ladder that
    grows after construction; a weight set per row inside the control network's kernels; an enhancer per model; a glide on a
    bank with `models=`."""

    def __init__(self, model, n_streams, samplerate, block_time, crossfade_time, device, buffer_num=4, threshold_db=-45.0,
                 use_graph=True, use_phase_vocoder=False, units_encoder=None, f0_extractor=None, f0_min=50, f0_max=1100,
                 f0_dither=True, crepe_ckpt=None, max_mix=4, enhancer=None, enhancer_adaptive_key="auto", enhancer_max_key=12,
                 active_widths=None, models=None, model_widths=None, glide_breakpoints=None, pitch_breakpoints=None,
                 formant=False, tune=False, indices=None, retrieve_k=8, envelope=False, envelope_hop_seconds=0.01,
                 envelope_frames=4):
        # every refusal comes before anything is allocated or launched on the device
        self.S = int(n_streams)
        if self.S < 1:
            raise ValueError(f"StreamBank: n_streams must be at least 1, got {n_streams}")
        if glide_breakpoints is not None:
            if isinstance(glide_breakpoints, bool) or not isinstance(glide_breakpoints, int) or not 1 <= glide_breakpoints <= MAX_GLIDE_POINTS:
                raise ValueError(f"StreamBank: glide_breakpoints must be an int in 1..{MAX_GLIDE_POINTS}, got {glide_breakpoints!r}")
            if models is not None:
                raise ValueError("StreamBank: glide_breakpoints= with models= is not supported (the per-model row gather moves a mix "
                                 "per row, not per frame)")
        if pitch_breakpoints is not None and (isinstance(pitch_breakpoints, bool) or not isinstance(pitch_breakpoints, int) or
                                              not 1 <= pitch_breakpoints <= MAX_GLIDE_POINTS):
            raise ValueError(f"StreamBank: pitch_breakpoints must be an int in 1..{MAX_GLIDE_POINTS}, got {pitch_breakpoints!r}")
        if not isinstance(formant, bool):
            raise ValueError(f"StreamBank: formant must be True or False, got {formant!r}")
        if not isinstance(tune, bool):
            raise ValueError(f"StreamBank: tune must be True or False, got {tune!r}")
        if indices is not None:
            if not isinstance(indices, UnitIndexBank):
                raise ValueError(f"StreamBank: indices must be an infer_offline.UnitIndexBank or None, got {type(indices).__name__}")
            if isinstance(retrieve_k, bool) or not isinstance(retrieve_k, int) or not 1 <= retrieve_k <= hipddsp.MAX_RETRIEVE_K:
                raise ValueError(f"StreamBank: retrieve_k must be an int in 1..{hipddsp.MAX_RETRIEVE_K}, got {retrieve_k!r}")
            n_unit = _model_field(models[0] if model is None and isinstance(models, (tuple, list)) and models else model, "n_unit")
            if indices.channels != n_unit:
                raise ValueError(f"StreamBank: the indices hold units of {indices.channels} channels, the model takes {n_unit}")
        if not isinstance(envelope, bool):
            raise ValueError(f"StreamBank: envelope must be True or False, got {envelope!r}")
        self.envelope_setting = None
        if envelope:
            if models is not None:
                raise ValueError("StreamBank: envelope=True with models= is not supported (the signal is rendered per model, "
                                 "behind the block that holds the envelope mix)")
            if units_encoder is None or f0_extractor is None:
                raise ValueError("StreamBank: envelope=True needs units_encoder= and f0_extractor= (the mix runs in push_audio's "
                                 "block)")
            try:
                one = EnvelopeMix(1.0, envelope_hop_seconds, envelope_frames)
                self.envelope_setting = (one.setting(samplerate), one.setting(_model_field(model, "sampling_rate")), one.frames)
            except ValueError as e:
                raise ValueError(f"StreamBank: {e}") from None
        if formant and models is not None:
            raise ValueError("StreamBank: formant=True with models= is not supported (the per-model row mover indexes the call's "
                             "rows, the formant row is indexed by slot)")
        self.glide_breakpoints, self.pitch_breakpoints = glide_breakpoints, pitch_breakpoints
        self.active_widths = None if active_widths is None else _check_active_widths(active_widths, self.S)
        if models is None and model_widths is not None:
            raise ValueError("StreamBank: model_widths= needs models=")
        self.model_widths = None
        if models is not None:
            self.model_widths = default_model_widths(self.S) if model_widths is None else \
                _check_active_widths(model_widths, self.S, "model_widths")
        self.models = [m.eval() for m in _check_models(model, models)]
        self.model_of_slot = [0] * self.S                            # host state: the model of every slot (`set_model`)
        model = self.models[0]
        self.max_mix = int(max_mix)
        if not 1 <= self.max_mix <= hipddsp.MAX_MIX:
            raise ValueError(f"StreamBank: max_mix must be in 1..{hipddsp.MAX_MIX}, got {max_mix}")
        self.model = model
        self.device = torch.device(device)
        self.block_size = int(model.block_size)
        self.model_sr = int(model.sampling_rate)
        self.n_spk = int(model.unit2ctrl.n_spk)
        self.samplerate = samplerate
        self.hop = self.block_size
        z = bank_sizes(samplerate, block_time, crossfade_time, buffer_num, self.block_size, self.model_sr)
        self.block, self.xfade, self.search, self.delay = z["block"], z["xfade"], z["search"], z["delay"]
        self.n_in, self.hop_size, self.frames, self.silence_front = z["n_in"], z["hop_size"], z["frames"], z["silence_front"]
        self.threshold_db = float(threshold_db)
        _check_analysers("StreamBank", "this bank's windows are", units_encoder, f0_extractor, samplerate, self.hop_size,
                         self.models)
        self.enhancer, self.enhancer_max_key, self.enhancer_plan = enhancer, enhancer_max_key, None
        self.out_sr = output_rate(self.model_sr, enhancer)
        if enhancer is not None:
            if isinstance(enhancer_max_key, bool) or not isinstance(enhancer_max_key, int) or not 0 <= enhancer_max_key <= 12:
                raise ValueError(f"StreamBank: enhancer_max_key must be an int in 0..12, got {enhancer_max_key!r}")
            request = enhancer.check_key_request(enhancer_adaptive_key, enhancer_max_key, "StreamBank: enhancer_adaptive_key")
            # (host integers only: the working rate and the lengths of every key; refuses rates the resampler cannot pair)
            self.enhancer_plan = enhancer.keyed_plan(self.frames * self.block_size, self.frames, self.model_sr, self.block_size,
                                                     self.silence_front, enhancer_max_key)
        _check_resample("StreamBank", self.out_sr, samplerate)
        if enhancer is not None:
            ends = [hipddsp.resample_length(n, self.out_sr, samplerate) for n in self.enhancer_plan.n_out]
            self.n_tail = self.block + self.xfade + self.search + self.delay
            if min(ends) < self.n_tail:
                raise ValueError(f"StreamBank: the enhancer returns {min(ends)} samples at {samplerate} Hz for some key, the splice "
                                 f"needs {self.n_tail}")
        f0_extractor = _f0_extractor(f0_extractor, samplerate, self.hop_size, f0_min, f0_max, crepe_ckpt, self.device)
        self.units_encoder, self.f0_extractor, self.f0_dither = units_encoder, f0_extractor, bool(f0_dither)
        dev = self.device
        self.windows = torch.zeros(self.S, self.n_in, device=dev)
        self._splicer_args = (samplerate, block_time, crossfade_time, dev, 0.01, 0.02, use_phase_vocoder)
        self.splicer = Splicer(*self._splicer_args, rows=self.S)
        self.sola_buffer = self.splicer.buffer                       # (S, xfade): the very tensor the splice updates
        self.spk_ids = torch.ones(self.S, self.max_mix, dtype=torch.int32, device=dev)   # every slot starts as speaker 1
        self.spk_w = torch.zeros(self.S, self.max_mix, device=dev)
        self.spk_w[:, 0] = 1.0
        self.pitch = torch.ones(self.S, device=dev)
        self.glide_clock = self.glide_n = self.glide_t = self.glide_w = None
        if glide_breakpoints is not None:                            # a clock and a timeline per slot (`set_timeline`)
            self.glide_clock = torch.zeros(self.S, dtype=torch.int64, device=dev)
            self.glide_n = torch.zeros(self.S, dtype=torch.int32, device=dev)
            self.glide_t = torch.zeros(self.S, glide_breakpoints, dtype=torch.int64, device=dev)
            self.glide_w = torch.zeros(self.S, glide_breakpoints, self.max_mix, device=dev)
        self.key_clock = self.key_n = self.key_t = self.key_semi = self.key_fac = None
        if pitch_breakpoints is not None:                            # a clock and a key timeline per slot (`set_pitch_timeline`)
            self.key_clock = torch.zeros(self.S, dtype=torch.int64, device=dev)
            self.key_n = torch.zeros(self.S, dtype=torch.int32, device=dev)
            self.key_t = torch.zeros(self.S, pitch_breakpoints, dtype=torch.int64, device=dev)
            self.key_semi = torch.zeros(self.S, pitch_breakpoints, device=dev)
            self.key_fac = torch.ones(self.S, pitch_breakpoints, device=dev)
        self.formant = torch.ones(self.S, device=dev) if formant else None    # a factor per slot (`set_formant`)
        self.tune_mask = self.tune_param = None                      # a setting per slot (`set_tune`), off: no bit of the mask
        if tune:
            self.tune_mask = torch.zeros(self.S, dtype=torch.int32, device=dev)
            self.tune_param = torch.tensor([[440.0, 0.0, 1.0]] * self.S, dtype=torch.float64).to(dev)
        self.indices, self.retrieve_k = indices, int(retrieve_k)     # the voices' stored units (`set_index`), every slot off at first
        self.index_of_slot = self.ratio_of_slot = None
        if indices is not None:
            if indices.device != torch.device(dev) and indices.device != torch.zeros(0, device=dev).device:
                raise ValueError(f"StreamBank: the indices live on {indices.device}, the bank on {dev}")
            self.index_of_slot = torch.full((self.S,), -1, dtype=torch.int32, device=dev)
            self.ratio_of_slot = torch.zeros(self.S, dtype=torch.float32, device=dev)
            indices.reserve(self.S, self.frames, self.retrieve_k)    # (an allocation: in front of every capture)
        # the envelope mix: a rate per slot (`set_envelope`), 1: off
        self.rate_of_slot = torch.ones(self.S, dtype=torch.float64, device=dev) if envelope else None
        self._resamplers = {}
        self.last_f0 = self.last_units = self.last_volume = self.last_shift = self.last_signal = self.last_key = None
        self.last_mix_w = None           # (A, Fr, max_mix): the block's per-frame weights on a bank with `glide_breakpoints`
        self.last_pitch = None           # (A, Fr): the block's per-frame f0 factors on a bank with `pitch_breakpoints`
        if enhancer is not None:
            self.enhancer_request = torch.full((self.S,), request, dtype=torch.int32, device=dev)   # -1 = 'auto', per slot
            self._n_end_by_key = torch.tensor(ends, dtype=torch.int32).to(dev)
            self._tail_idx = torch.arange(self.n_tail, device=dev)
        self.use_graph = bool(use_graph)
        self.graph = None                # the synthesis graph of `push_block` (a bank without the analysers)
        self.bank_graph = None           # the whole-block graph of `push_audio`
        self.enhancer_graph = None       # the enhancer stage, replayed right after either of them
        self.graph_builds = 0
        self.last_active = None          # the slots of the last call that named them (`active=`)
        self._full = _Rows(self, self.S, compact=False)
        self._compact = {W: _Rows(self, W, compact=True) for W in self.active_widths or ()}
        self._batch = self._sig = self._model_rows = None            # a bank with `models=`: see `_render_models`
        if self.model_widths is not None:
            import graphed
            T, n_unit = self.frames * self.block_size, int(model.unit2ctrl.n_unit)
            self._batch = {"units": torch.zeros(self.S, self.frames, n_unit, device=dev), "f0": torch.zeros(self.S, self.frames, 1, device=dev),
                           "volume": torch.zeros(self.S, self.frames, device=dev), "noise": torch.zeros(self.S, T, device=dev),
                           "mix": (torch.ones(self.S, self.max_mix, dtype=torch.int32, device=dev), torch.zeros(self.S, self.max_mix, device=dev))}
            self._sig = torch.zeros(self.S, T, device=dev)
            self._model_rows = [{W: graphed.GraphedModelRows(m, W, self.frames, self._batch, self._sig, self.threshold_db,
                                                             capture=self.use_graph) for W in self.model_widths} for m in self.models]
            self.graph_builds += len(self.models) * len(self.model_widths) * int(self.use_graph)
        if self.use_graph:
            self._capture(self._full)
            self.graph, self.bank_graph, self.enhancer_graph = self._full.graph, self._full.bank_graph, self._full.enhancer_graph
            for rows in self._compact.values():
                self._capture(rows)

    def _capture(self, rows):
        """The chain at the width of `rows` as its graphs: the block (or the synthesis alone) and the enhancer stage together
        count as one build."""
        import graphed
        shared = self.model_widths is None                           # (with `models=` the synthesis is `_render_models`'s)
        if self.f0_extractor is not None:
            rows.bank_graph = graphed.GraphedBlock(
                self.model if shared else None, self.units_encoder, self.f0_extractor, rows.windows, self.block, self.samplerate, self.hop_size,
                self.silence_front, rows.pitch_term, self.threshold_db, mix_rows=rows.mix, f0_dither=self.f0_dither, push=rows.push,
                keep=[c for c in (self.glide_clock, self.key_clock) if c is not None],   # (the capture's runs advance the clocks)
                **({} if self.formant is None else {"formant": rows.formant_term}),
                **({} if self.tune_mask is None else {"tune": rows.tune_term}),
                **({} if self.indices is None else {"retrieve": rows.retrieve_term}),
                **({} if self.rate_of_slot is None else {"envelope": rows.envelope_term}))
        elif shared:
            rows.graph = graphed.GraphedSynth(self.model, rows.W, self.frames, spk_mix_rows=rows.mix,
                                              **({} if self.formant is None else {"formant": rows.formant_term}))
        if self.enhancer is not None:
            rows.enhancer_graph = graphed.GraphedBankEnhancer(
                self.enhancer, self.enhancer_plan, rows.W, rows.request, self.model_sr, self.block_size, self.samplerate,
                self._n_end_by_key, self._tail_idx)
        self.graph_builds += 1

    def _rows_for(self, active):
        """`active` of a push call -> (the rows the call runs on, A, the slots as a tuple or None): every refusal, on the host."""
        if active is None:
            return self._full, self.S, None
        if self.active_widths is None:
            raise ValueError("StreamBank: active= needs a bank built with active_widths=")
        try:
            active = list(active)
        except TypeError:
            raise ValueError(f"StreamBank: active must be a sequence of slots, got {active!r}") from None
        if not active:
            raise ValueError("StreamBank: active names at least one slot (an empty call advances nothing)")
        if any(isinstance(s, bool) or not isinstance(s, int) or not 0 <= s < self.S for s in active):
            raise ValueError(f"StreamBank: active holds slot ints in [0, {self.S}), got {active!r}")
        if any(a >= b for a, b in zip(active, active[1:])):
            raise ValueError(f"StreamBank: active must be strictly increasing, got {active!r}")
        return self._compact[active_width(len(active), self.active_widths)], len(active), tuple(active)

    def _check_draws(self, noise, rand_ini, A):
        """`noise` / `rand_ini` of a call with `active`: compact like every per-row argument."""
        if noise is not None and tuple(noise.shape) != (A, self.frames * self.block_size):
            raise ValueError(f"StreamBank: noise (A, Fr * block_size) = {(A, self.frames * self.block_size)}, got {tuple(noise.shape)}")
        if rand_ini is not None and tuple(rand_ini.shape) not in ((9,), (A, 9)):
            raise ValueError(f"StreamBank: rand_ini (9,) or (A, 9) = {(A, 9)}, got {tuple(rand_ini.shape)}")

    def _slot(self, slot):
        if isinstance(slot, bool) or not isinstance(slot, int) or not 0 <= slot < self.S:
            raise ValueError(f"StreamBank: slot must be an int in [0, {self.S}), got {slot!r}")
        return slot

    def set_speaker(self, slot, spk_id=None, spk_mix_dict=None):
        """Slot `slot` sings as `spk_mix_dict` ({speaker id: weight}, 1 to `max_mix` ids) or as the plain `spk_id` (the row
        {id: 1.0}) from the next block on: one write to that slot's rows of the two device tables, no capture."""
        slot = self._slot(slot)
        if (spk_id is None) == (spk_mix_dict is None):
            raise ValueError("StreamBank.set_speaker: pass spk_id or spk_mix_dict (one of them)")
        self._write_mix(slot, *self._mix_tables(self.model_of_slot[slot], spk_id, spk_mix_dict))

    def _mix_tables(self, k, spk_id, spk_mix_dict):
        """The mix row of a slot on model `k` as CPU tables (ids (1, K), w (1, K)); ids are checked against THAT model's `n_spk`."""
        n_spk = int(self.models[k].unit2ctrl.n_spk)
        if spk_mix_dict is not None:
            mix = {int(i): float(v) for i, v in spk_mix_dict.items()}
            if not 1 <= len(mix) <= self.max_mix:
                raise ValueError(f"StreamBank: a speaker mix holds 1 to max_mix = {self.max_mix} ids, got {len(mix)}")
        else:
            mix = {int(spk_id): 1.0}
        if any(not 1 <= i <= n_spk for i in mix):
            raise ValueError(f"StreamBank: speaker ids must be in [1, {n_spk}], got {sorted(mix)}")
        return hipddsp.mix_rows([mix], self.max_mix, n_spk)

    def _write_mix(self, slot, ids, w):
        self.spk_ids[slot].copy_(ids[0])
        self.spk_w[slot].copy_(w[0])
        if self.glide_n is not None:                                 # a plain speaker ends a glide
            self.glide_n[slot:slot + 1].zero_()

    def set_timeline(self, slot, timeline, at=0.0):
        """Slot `slot` glides along `timeline` (an `infer_offline.SpeakerTimeline`) from the next block on, in STREAM time: time 0
        is the first sample pushed after this call, or `at` seconds into the timeline with `at=`.  Breakpoint n sits at
        int(round(seconds * samplerate)) device samples.  Frames of the window that are older than time 0 hold the first
        breakpoint's weights, frames behind the last breakpoint its weights.  Writes the slot's `spk_ids` row (the timeline's `ids`,
        padded with id 1), its rows of `glide_t` / `glide_w`, `glide_n` and `glide_clock`: device rows only, no capture.
        ValueError, before any write: a bank built without `glide_breakpoints`, more points than it, two points on one sample,
        more ids than `max_mix`, an id outside [1, n_spk] of the slot's model."""
        if self.glide_breakpoints is None:
            raise ValueError("StreamBank.set_timeline: this bank was built without glide_breakpoints=")
        slot = self._slot(slot)
        if not isinstance(timeline, SpeakerTimeline):
            raise ValueError(f"StreamBank.set_timeline: timeline must be an infer_offline.SpeakerTimeline, got {type(timeline).__name__}")
        if isinstance(at, bool) or not isinstance(at, (int, float)) or at != at or abs(at) == float("inf"):
            raise ValueError(f"StreamBank.set_timeline: at must be a finite number of seconds, got {at!r}")
        times = [int(round(t * self.samplerate)) for t, _ in timeline.points]
        if len(times) > self.glide_breakpoints:
            raise ValueError(f"StreamBank.set_timeline: {len(times)} points, the bank holds glide_breakpoints = {self.glide_breakpoints} "
                             f"per slot")
        for n in range(1, len(times)):
            if times[n] <= times[n - 1]:
                raise ValueError(f"StreamBank.set_timeline: points {n - 1} and {n} ({timeline.points[n - 1][0]} s, "
                                 f"{timeline.points[n][0]} s) both land on sample {times[n]} at {self.samplerate} Hz")
        ids = list(timeline.ids)
        if len(ids) > self.max_mix:
            raise ValueError(f"StreamBank.set_timeline: the timeline names {len(ids)} ids, a mix holds max_mix = {self.max_mix}")
        n_spk = int(self.models[self.model_of_slot[slot]].unit2ctrl.n_spk)
        if any(not 1 <= i <= n_spk for i in ids):
            raise ValueError(f"StreamBank.set_timeline: speaker ids must be in [1, {n_spk}], got {sorted(ids)}")
        P, K = self.glide_breakpoints, self.max_mix
        row_ids = torch.tensor(ids + [1] * (K - len(ids)), dtype=torch.int32)
        row_t = torch.tensor(times + [0] * (P - len(times)), dtype=torch.int64)
        row_w = torch.zeros(P, K)
        for n, (_, mix) in enumerate(timeline.points):
            for k, i in enumerate(ids):
                row_w[n, k] = mix.get(i, 0.0)
        self.spk_ids[slot].copy_(row_ids)
        self.glide_t[slot].copy_(row_t)
        self.glide_w[slot].copy_(row_w)
        self.glide_n[slot:slot + 1].fill_(len(times))
        self.glide_clock[slot:slot + 1].fill_(int(round(at * self.samplerate)))

    def set_model(self, slot, k, spk_id=1, spk_mix_dict=None):
        """Slot `slot` is rendered by `models[k]` from the next block on, as speaker `spk_id` of that model or as `spk_mix_dict`
        (which then replaces `spk_id`): ids are checked against that model's `n_spk`, and the slot's old speaker does not carry
        over (it may not exist there).  Host state (`model_of_slot`) and one write to the slot's mix rows; nothing is captured.
        Window, SOLA buffer, pitch and key request stay, as does the model under `reset(slot)`."""
        slot = self._slot(slot)
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < len(self.models):
            raise ValueError(f"StreamBank.set_model: k must be an int in [0, {len(self.models)}), got {k!r}")
        tables = self._mix_tables(k, spk_id, spk_mix_dict)
        self.model_of_slot[slot] = k
        self._write_mix(slot, *tables)

    def set_pitch(self, slot, semitones):
        """Slot `slot` is shifted by `semitones` from the next block on (f0 * 2 ** (semitones / 12)): one device write.  On a bank
        with `pitch_breakpoints` it ends the slot's key timeline."""
        slot = self._slot(slot)
        self.pitch[slot:slot + 1].fill_(2 ** (float(semitones) / 12))
        if self.key_n is not None:
            self.key_n[slot:slot + 1].zero_()

    def set_formant(self, slot, semitones):
        """Slot `slot`'s formants are shifted by `semitones` (|s| <= 24, positive: brighter) at the same pitch from the next block
        on: one write of 2 ** (semitones / 12) to the slot's row of `formant`, no capture.  ValueError on a bank built without
        `formant=True`, or for a shift that is no finite number within +-24."""
        if self.formant is None:
            raise ValueError("StreamBank.set_formant: this bank was built without formant=True")
        slot = self._slot(slot)
        self.formant[slot:slot + 1].fill_(hipddsp.formant_factor(semitones))

    def set_tune(self, slot, tune):
        """Slot `slot`'s f0 is pulled toward the notes of `tune` (an `infer_offline.PitchTune`) from the next block on, None
        switches it off: one write to the slot's rows of `tune_mask` and `tune_param`, no capture.  ValueError on a bank built
        without `tune=True`, or for anything but a PitchTune or None."""
        if self.tune_mask is None:
            raise ValueError("StreamBank.set_tune: this bank was built without tune=True")
        if tune is not None and not isinstance(tune, PitchTune):
            raise ValueError(f"StreamBank.set_tune: tune must be an infer_offline.PitchTune or None, got {tune!r}")
        slot = self._slot(slot)
        mask, param = (0, (440.0, 0.0, 1.0)) if tune is None else tune.setting(self.hop_size / self.samplerate)
        self.tune_mask[slot:slot + 1].fill_(mask)
        self.tune_param[slot:slot + 1].copy_(torch.tensor([param], dtype=torch.float64))

    def set_envelope(self, slot, rate):
        """Slot `slot`'s output keeps the share `rate` in [0, 1] of its own loudness envelope and takes the rest from its input's
        from the next block on (RVC's `rms_mix_rate`); None - or 1 - switches it off: one write to the slot's row of
        `rate_of_slot`, no capture.  ValueError on a bank built without `envelope=True`, or for a rate outside [0, 1]."""
        if self.rate_of_slot is None:
            raise ValueError("StreamBank.set_envelope: this bank was built without envelope=True")
        if rate is not None:
            try:
                rate = EnvelopeMix(rate).rate
            except ValueError as e:
                raise ValueError(f"StreamBank.set_envelope: {e}") from None
        slot = self._slot(slot)
        self.rate_of_slot[slot:slot + 1].fill_(1.0 if rate is None else rate)

    def set_index(self, slot, index, ratio=0.5):
        """Slot `slot`'s units are blended with their nearest stored units of index number `index` of the bank's `indices`
        from the next block on, at `ratio` in [0, 1]; None switches it off: one write to the slot's rows of `index_of_slot` and
        `ratio_of_slot`, no capture.  ValueError on a bank built without `indices=`, for an index number outside the bank or a
        ratio that is not a finite number in [0, 1]."""
        if self.indices is None:
            raise ValueError("StreamBank.set_index: this bank was built without indices=")
        if index is not None:
            check_job_index("StreamBank.set_index", (index, ratio), len(self.indices))
        slot = self._slot(slot)
        self.index_of_slot[slot:slot + 1].fill_(-1 if index is None else int(index))
        self.ratio_of_slot[slot:slot + 1].fill_(0.0 if index is None else float(ratio))

    def set_pitch_timeline(self, slot, timeline, at=0.0):
        """Slot `slot`'s key follows `timeline` (an `infer_offline.KeyTimeline`) from the next block on, in STREAM time, as
        `set_timeline` has it for the voice: time 0 is the first sample pushed after this call, or `at` seconds into the timeline
        with `at=`; a point at t seconds sits at int(round(t * samplerate)) device samples.  Frames of the window older than the
        first point hold its key, frames behind the last point the last one's; between two the key is linear in semitones.
        Writes the slot's rows of `key_t` / `key_semi` / `key_fac`, `key_n` and `key_clock`: device rows only, no capture.
        `set_pitch` ends the timeline.  ValueError, before any write: a bank built without `pitch_breakpoints`, more points than
        it, two points on one sample."""
        if self.pitch_breakpoints is None:
            raise ValueError("StreamBank.set_pitch_timeline: this bank was built without pitch_breakpoints=")
        slot = self._slot(slot)
        if not isinstance(timeline, KeyTimeline):
            raise ValueError(f"StreamBank.set_pitch_timeline: timeline must be an infer_offline.KeyTimeline, got "
                             f"{type(timeline).__name__}")
        if isinstance(at, bool) or not isinstance(at, (int, float)) or at != at or abs(at) == float("inf"):
            raise ValueError(f"StreamBank.set_pitch_timeline: at must be a finite number of seconds, got {at!r}")
        times = [int(round(t * self.samplerate)) for t, _ in timeline.points]
        if len(times) > self.pitch_breakpoints:
            raise ValueError(f"StreamBank.set_pitch_timeline: {len(times)} points, the bank holds pitch_breakpoints = "
                             f"{self.pitch_breakpoints} per slot")
        for n in range(1, len(times)):
            if times[n] <= times[n - 1]:
                raise ValueError(f"StreamBank.set_pitch_timeline: points {n - 1} and {n} ({timeline.points[n - 1][0]} s, "
                                 f"{timeline.points[n][0]} s) both land on sample {times[n]} at {self.samplerate} Hz")
        pad = self.pitch_breakpoints - len(times)
        keys = [key for _, key in timeline.points]
        self.key_t[slot].copy_(torch.tensor(times + [0] * pad, dtype=torch.int64))
        self.key_semi[slot].copy_(torch.tensor(keys + [0.0] * pad, dtype=torch.float32))
        self.key_fac[slot].copy_(torch.tensor([2 ** (float(k) / 12) for k in keys] + [1.0] * pad, dtype=torch.float32))
        self.key_n[slot:slot + 1].fill_(len(times))
        self.key_clock[slot:slot + 1].fill_(int(round(at * self.samplerate)))

    def set_enhancer_key(self, slot, key):
        """Slot `slot` is enhanced with the adaptive key `key` (a whole number in 0..enhancer_max_key) or by the 'auto' rule from
        the next block on: one write to that slot's row of the device request table, no capture."""
        slot = self._slot(slot)
        if self.enhancer is None:
            raise ValueError("StreamBank.set_enhancer_key: this bank was built without enhancer=")
        request = self.enhancer.check_key_request(key, self.enhancer_max_key, "StreamBank.set_enhancer_key: key")
        self.enhancer_request[slot:slot + 1].fill_(request)

    def reset(self, slot):
        """A new caller takes slot `slot`: its window and its SOLA buffer are zeroed (model, speaker and pitch stay as set).  On
        a bank with `glide_breakpoints` the slot's clock is zeroed too and its timeline stays: the glide starts from its beginning;
        on one with `pitch_breakpoints` the key clock and the key timeline likewise.  On a bank with `formant` the slot's formant
        factor goes back to 1, on one with `tune` the slot's pitch correction is switched off, on one with `indices` its
        unit retrieval, on one with `envelope` its envelope mix."""
        slot = self._slot(slot)
        self.windows[slot].zero_()
        self.sola_buffer[slot].zero_()
        if self.glide_clock is not None:
            self.glide_clock[slot:slot + 1].zero_()
        if self.key_clock is not None:
            self.key_clock[slot:slot + 1].zero_()
        if self.formant is not None:
            self.formant[slot:slot + 1].fill_(1.0)
        if self.tune_mask is not None:
            self.tune_mask[slot:slot + 1].zero_()
        if self.indices is not None:
            self.index_of_slot[slot:slot + 1].fill_(-1)
            self.ratio_of_slot[slot:slot + 1].zero_()
        if self.rate_of_slot is not None:
            self.rate_of_slot[slot:slot + 1].fill_(1.0)

    def _check_blocks(self, blocks, A, rows="S"):
        if not isinstance(blocks, torch.Tensor) or tuple(blocks.shape) != (A, self.block):
            got = tuple(blocks.shape) if isinstance(blocks, torch.Tensor) else type(blocks).__name__
            raise ValueError(f"StreamBank: a call takes blocks of shape ({rows}, block) = {(A, self.block)}, got {got}")

    def _enhanced_tail(self, rows, sig, f0, rand_ini):
        """Steps 6-7 with the enhancer: -> every row's own tail (W, block + xfade + search + delay) at the device rate."""
        if rows.enhancer_graph is not None:
            tail, key = rows.enhancer_graph(sig, f0, rand_ini)
        else:
            import graphed
            if rand_ini is None:
                rand_ini = torch.rand(rows.W, 9, device=self.device)
            tail, key = graphed.bank_enhancer_chain(
                hipddsp.context_for(self.device), self.enhancer, self.enhancer_plan, sig, f0, rows.request,
                rand_ini.to(self.device), self.model_sr, self.block_size, self.samplerate, self._n_end_by_key, self._tail_idx)
        self.last_key, = rows.real(key)
        return tail

    def _render_models(self, rows, slots, units, f0, volume, noise):
        """Step 4-5 of a bank with `models=`: the features of the call's rows (W, ...) go to the bank's staging tensors, then
        every model that owns a row of the call renders its rows: one replay of its compact chain (`graphed.GraphedModelRows`:
        gather by a device row table, forward with mix rows, gate, scatter) at the smallest width of `model_widths` that holds
        them.  A model without rows in the call is not replayed.  -> the gated signal (W, Fr * block_size) of the call.  Padding
        rows of the call belong to no model: their rows of the signal are whatever an earlier call left there."""
        import graphed
        b, W = self._batch, rows.W
        for name, t in (("units", units), ("f0", f0), ("volume", volume)):
            b[name][:W].copy_(t.reshape(b[name][:W].shape))
        graphed._refill(b["noise"][:W], noise)
        b["mix"][0][:W].copy_(rows.spk_ids)
        b["mix"][1][:W].copy_(rows.spk_w)
        owned = {}
        for r, slot in enumerate(range(self.S) if slots is None else slots):
            owned.setdefault(self.model_of_slot[slot], []).append(r)
        for k in sorted(owned):
            self._model_rows[k][active_width(len(owned[k]), self.model_widths)](owned[k])
        return self._sig[:W]

    def _splice(self, rows, sig, f0=None, rand_ini=None):
        """Steps 6-8 over the rows: (W, Fr * block_size) at the model's rate -> (A, block) samples to play; the spliced buffers
        of a compact batch go back to their slots."""
        if rand_ini is not None and rows.rows is not None and rand_ini.dim() == 2:
            rand_ini = rows.pad(rand_ini.to(self.device))
        if self.enhancer is not None:
            sig = self._enhanced_tail(rows, sig, f0, rand_ini).contiguous()
        else:
            sig = _to_device_rate(self._resamplers, sig, self.model_sr, self.samplerate).contiguous()
        emitted = rows.splicer.push(sig)
        rows.scatter()
        self.last_signal, self.last_shift, emitted = rows.real(sig, rows.splicer.last_shift, emitted)
        return emitted

    @torch.no_grad()
    def push_audio(self, blocks, noise=None, rand_ini=None, active=None):
        """blocks (S, block) raw samples at the device rate, one block per stream -> (S, block) samples to play.  `noise`
        (S, Fr * block_size) in [0, 1) replaces the fresh draw and `rand_ini` (9,) or (S, 9) the enhancer's source phases
        (parity tests).  With `active` (A slots, strictly increasing) every per-row argument and the result have A rows, row r
        belonging to slot active[r]; the other slots stay as they are (class docstring)."""
        if self.f0_extractor is None:
            raise ValueError("StreamBank: push_audio needs units_encoder= and f0_extractor= at construction")
        rows, A, active = self._rows_for(active)
        self._check_blocks(blocks, A, "S" if active is None else "A")
        if active is not None:
            self._check_draws(noise, rand_ini, A)
            noise = None if noise is None else rows.pad(noise.to(self.device))
        blocks = rows.pad(blocks.to(self.device, torch.float32).contiguous())
        rows.select(active)
        if rows.bank_graph is not None:
            sig, f0, units, volume = rows.bank_graph(blocks, noise=noise)
        else:
            import graphed
            sig, f0, units, volume = graphed.block_chain(
                hipddsp.context_for(self.device), self.model if self._model_rows is None else None, self.units_encoder,
                self.f0_extractor, rows.windows, blocks, self.samplerate, self.hop_size, self.silence_front, rows.pitch_term,
                self.threshold_db, self.hop,
                {"spk_id": None, "spk_mix_rows": rows.mix, **({} if self.formant is None else {"formant": rows.formant_term})},
                noise, self.f0_dither, push=rows.push, **({} if self.tune_mask is None else {"tune": rows.tune_term}),
                **({} if self.indices is None else {"retrieve": rows.retrieve_term}),
                **({} if self.rate_of_slot is None else {"envelope": rows.envelope_term}))
        if self._model_rows is not None:
            sig = self._render_models(rows, active, units, f0, volume, noise)
        self.last_f0, self.last_units, self.last_volume = rows.real(f0, units, volume)
        if rows.w_frames is not None:
            self.last_mix_w, = rows.real(rows.w_frames)
        if rows.pitch_frames is not None:
            self.last_pitch, = rows.real(rows.pitch_frames)
        self.last_active = active
        return self._splice(rows, sig, f0, rand_ini)

    @torch.no_grad()
    def push_block(self, blocks, units, f0, noise=None, rand_ini=None, active=None):
        """The analysis-free form: blocks (S, block), and `units` (S, Fr, C) and `f0` (S, Fr, 1) of the CURRENT windows from the
        caller (before the pitch factor, which is applied here) -> (S, block) samples to play.  `active`: as in `push_audio`."""
        rows, A, active = self._rows_for(active)
        self._check_blocks(blocks, A, "S" if active is None else "A")
        if self.f0_extractor is not None:
            raise ValueError("StreamBank: this bank was built for push_audio; build one without units_encoder / f0_extractor "
                             "for push_block (one capture per bank)")
        if tuple(units.shape[:2]) != (A, self.frames) or tuple(f0.shape) != (A, self.frames, 1):
            raise ValueError(f"StreamBank: units (S, Fr, C) and f0 (S, Fr, 1) with (S, Fr) = {(A, self.frames)}, got "
                             f"{tuple(units.shape)} and {tuple(f0.shape)}")
        if active is not None:
            self._check_draws(noise, rand_ini, A)
            noise = None if noise is None else rows.pad(noise.to(self.device))
        blocks = rows.pad(blocks.to(self.device, torch.float32).contiguous())
        ctx = hipddsp.context_for(self.device)
        rows.select(active)
        rows.push(ctx, rows.windows, blocks)
        units = rows.pad(units.to(self.device))
        f0 = rows.pad(f0.to(self.device, torch.float32)) * \
            (rows.pitch[:, None, None] if rows.pitch_frames is None else rows.pitch_frames[:, :, None])
        if self.tune_mask is not None:
            ctx.f0_tune_(f0, *rows.tune_term[:2], owner=rows.rows)
        volume = ctx.volume_extract(rows.windows, self.hop_size)
        if self._model_rows is not None:
            sig = self._render_models(rows, active, units, f0, volume, noise)
        else:
            if rows.graph is not None:
                sig = rows.graph(units, f0, volume, None, noise=noise)[0]
            else:
                kw = {} if noise is None else {"noise": noise}
                if self.formant is not None:
                    kw["formant"] = rows.formant_term
                sig = (self.model if self.formant is None else self.model.forward_formant)(
                    units, f0, volume, None, spk_mix_rows=rows.mix, **kw)[0]
            ctx.volume_gate_(sig, volume, self.threshold_db, self.hop)
        self.last_f0, self.last_units, self.last_volume = rows.real(f0, units, volume)
        if rows.w_frames is not None:
            self.last_mix_w, = rows.real(rows.w_frames)
        if rows.pitch_frames is not None:
            self.last_pitch, = rows.real(rows.pitch_frames)
        self.last_active = active
        return self._splice(rows, sig, f0, rand_ini)
