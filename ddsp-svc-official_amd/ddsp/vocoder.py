"""Drop-in for the synthesiser half of the reference's `ddsp/vocoder.py` (:335-550): `load_model`, `Sins`,
`CombSub`, `CombSubFast`, `DotDict`, with the same constructors, `forward(...)` signature, return tuple and
state-dict keys, executed by hand-written gfx950 kernels through libddsp_amd (no CPU fallback).

Differences a caller can observe, all additive:
  * `forward(..., noise=None, noise_seed=None)`: the reference draws its noise excitation from the CPU
    mt19937 stream (`torch.rand_like`), which a GPU cannot reproduce.  `noise` (B,T) U[0,1) injects the
    draw (parity runs); otherwise a counter-based in-kernel generator is used, seeded from torch's default
    generator (so `torch.manual_seed` still makes a run repeatable) or from `noise_seed`.
  * `c=True` (causal convolutions + causal linear attention): forward and training; the two third-party primitives
    behind it are restated from their definitions.
  * `forward(..., n_frames=None)`: a RAGGED batch.  `n_frames` (a sequence of B ints or a CPU integer tensor (B,),
    1 <= n_frames[b] <= Fr) gives the frames of each row inside the padded (B, Fr, ...) inputs; row b of every returned
    tensor is then, over its first n_frames[b] frames / n_frames[b] * block_size samples, what the model returns for that
    row alone at its own length, and exactly 0.0 after them.  What the padding of units / f0 / volume / noise holds (zeros,
    garbage, NaN) does not matter.  With `noise_seed=` the draw is repeatable but not the draw of the rows' solo calls.
    Training too: on a model in training mode (`model.train()`, as every training loop sets it) the call is recorded under
    grad mode like the one without counts, and the gradient of every parameter is the sum over rows of the gradient the
    model gives for that row alone (its inputs, noise and upstream gradients cropped to the row); what the upstream
    gradients hold past a row's end does not matter either.  A model in eval mode keeps the refusal it always had: with grad
    mode on and a parameter that wants a gradient a ragged call raises NotImplementedError (an inference caller that forgot
    torch.no_grad() would otherwise keep the activations of every call).
  * `forward(..., spk_mix_rows=(ids, w))`: a speaker mix PER ROW as device data.  `ids` (B, K) int32 (1-based) and `w`
    (B, K) fp32, 1 <= K <= 16, both on the model's device; row b adds sum_k w[b, k] * spk_embed[ids[b, k] - 1] in slot
    order.  A slot {id 1, weight 0} pads a shorter row, the row {id: 1.0} is a plain speaker id
    (`hipddsp.mix_rows` builds the tables).  `spk_id` is then ignored; together with `spk_mix_dict` it raises ValueError.
    The kernels read the tables when they run, so a captured graph follows edits to them
    (`graphed.GraphedSynth(..., spk_mix_rows=True)`, `realtime.StreamBank`).  Works with and without `n_frames=`.
    Inference only (NotImplementedError under grad mode).  An id outside [1, n_spk] in a device table is reported by the
    kernel through the context's device error word (ValueError from the next library call).
  * A speaker mix PER FRAME (a voice that glides inside a call): the pair (ids (B, K) int32, w (B, Fr, K) fp32) - the row
    mix with a frame axis in its weights; frame i of row b adds sum_k w[b, i, k] * spk_embed[ids[b, k] - 1].  It is passed
    as `spk_mix_rows=` (every model) or as `spk_mix_frames=` (`CombSub`, `CombSubFast`, which take extra keywords; `Sins`
    keeps the reference's closed parameter list).  A `spk_mix_dict` whose values are tensors of shape (B, Fr, 1), (1, Fr, 1)
    or (Fr,) - what the reference broadcasts in `x + v * spk_embed(id - 1)` - is turned into that form, slots in dict
    order; a dict of numbers behaves as ever.  With `n_frames=` the weights past a row's count do not matter.  Inference
    only, device error word and graph capture as for the row mix.
  * `forward_formant(units_frames, f0_frames, volume_frames, spk_id, formant, ...)`: `forward` with a FORMANT SHIFT - the
    spectral-envelope columns of the control matrix are stretched along the frequency axis between the control network and the
    filter synthesis (`ddsp_ctrl_warp`, one launch; DESIGN section 7 states the rule), so the timbre reads as a brighter or
    darker vocal tract at the same pitch.  `formant`: a number of semitones (|s| <= 24; positive raises the formants; the
    factor is 2 ** (s / 12) stored to fp32) or a fp32 device tensor of FACTORS, (B,) one per row or (B, Fr) one per frame; a
    pair (factors (S,), slot_of_row (B,) int32) reads row b's factor at factors[slot_of_row[b]] (an entry outside [0, S): a
    padding row, no shift - `realtime.StreamBank`).  Warped: `harmonic_magnitude` and `noise_magnitude` (CombSub, CombSubFast),
    `amplitudes` and `noise_magnitude` (Sins); `group_delay` and `harmonic_phase` are not.  The other parameters and the
    returned tuple are `forward`'s (`Sins`: without `max_upsample_dim`); 0 semitones and factors of 1 give `forward`'s bits.
    Inference only (NotImplementedError under grad mode); a factor that is not finite or not > 0 leaves its frames unshifted
    and is reported through the context's device error word.
"""
import os

import torch
import yaml

import hipddsp
from hipddsp import (COMB_SINC, COMB_SINC_GATED, COMB_NONE, EXC_AUDIO, EXC_GENERATE, EXC_UNIT_NOISE, FIR_ALLPASS,
                     FIR_DYNAMIC, FIR_STATIC, FIR_SPLIT_BF16)

# the analysers live in ddsp/analysis.py; their names stay importable from here
from .analysis import (Audio2CVec, Audio2CVec768, Audio2HubertSoft, F0_Extractor, Units_Encoder,  # noqa: F401
                       Volume_Extractor, _find_torchcrepe_checkpoint, align_units)
from .unit2control import Unit2Control, is_frame_mix


class DotDict(dict):
    """Attribute access to nested config dicts (reference `ddsp/vocoder.py:335-341`)."""

    def __getattr__(self, key):
        val = self.get(key)
        return DotDict(val) if type(val) is dict else val

    __setattr__ = dict.__setitem__
    __delattr__ = dict.__delitem__


def load_model(model_path, device="cpu"):
    """Reads `<dir>/config.yaml`, builds the model it names, loads `ckpt['model']`
    (reference `ddsp/vocoder.py:343-369`).  Returns (model.eval(), args)."""
    with open(os.path.join(os.path.split(model_path)[0], "config.yaml"), "r") as fh:
        args = DotDict(yaml.safe_load(fh))
    kind = args.model.type
    if kind == "Sins":
        model = Sins(sampling_rate=args.data.sampling_rate, block_size=args.data.block_size,
                     n_harmonics=args.model.n_harmonics, n_mag_allpass=args.model.n_mag_allpass,
                     n_mag_noise=args.model.n_mag_noise, n_unit=args.data.encoder_out_channels,
                     n_spk=args.model.n_spk, c=args.model.c)
    elif kind == "CombSub":
        model = CombSub(sampling_rate=args.data.sampling_rate, block_size=args.data.block_size,
                        n_mag_allpass=args.model.n_mag_allpass, n_mag_harmonic=args.model.n_mag_harmonic,
                        n_mag_noise=args.model.n_mag_noise, n_unit=args.data.encoder_out_channels,
                        n_spk=args.model.n_spk, c=args.model.c)
    elif kind == "CombSubFast":
        model = CombSubFast(sampling_rate=args.data.sampling_rate, block_size=args.data.block_size,
                            n_unit=args.data.encoder_out_channels, n_spk=args.model.n_spk, c=args.model.c)
    else:
        raise ValueError(f" [x] Unknown Model: {kind}")
    print(" [Loading] " + model_path)
    # weights_only: a checkpoint is {'global_step', 'model', 'optimizer'} of tensors (reference logger/saver.py:83-87)
    ckpt = torch.load(model_path, map_location=torch.device(device), weights_only=True)
    model.to(device)
    model.load_state_dict(ckpt["model"])
    model.eval()
    return model, args


class _SynthBase(torch.nn.Module):
    """What the three synthesisers share: one `forward` body (`_forward`) and the protocol of the autograd node.  A model
    states `_comb_mode` / `_front_wants` (the comb the phase scan writes, and `want_phase`: nowhere else) and supplies
    `_render` (its DSP chain, written once) and `_train_backward` (the chain's adjoint; `crop` from `_crop`, applied to a
    gradient wherever `_render` cropped the signal between two stages - the upstream gradients arrive cropped)."""

    def __init__(self, sampling_rate, block_size):
        super().__init__()
        self.register_buffer("sampling_rate", torch.tensor(sampling_rate))
        self.register_buffer("block_size", torch.tensor(block_size))
        self._sr = int(sampling_rate)
        self._hop = int(block_size)

    def _context(self, f0_frames, ragged=False):
        if not f0_frames.is_cuda:
            raise RuntimeError("the synthesiser runs on a HIP device only (no CPU fallback): move the model and its "
                               "inputs to 'cuda'")
        if ragged and self._hop % 4:
            raise ValueError("n_frames= needs a block_size that is a multiple of 4")
        return hipddsp.context_for(f0_frames.device)

    def _scan(self, ctx, f0_frames, initial_phase, infer):
        return ctx.phase_scan(f0_frames, self._hop, self._sr, initial_phase, bool(infer), self._comb_mode,
                              **self._front_wants)

    def _render(self, ctx, ctrl, ps, f0_frames, excitation, n_dev=None, keep=False):
        """The model's DSP chain: fused control matrix (B,Fr,sum) + phase-scan outputs `ps` -> (outputs, saved), for
        inference, ragged inference and the training forward alike.
        `excitation()` -> (nz, exc, seed) of the noise branch (`_noise_args` / `_ragged_noise`), called where the chain
        needs it: the ragged draw is a launch and a (B,T) tensor of its own.  `n_dev`: the counts of a ragged batch whose
        ctrl and f0 are held over the padding; every signal is then cropped to its row before it enters the next filter.
        `keep`: `saved` is what `_train_backward` needs (else None, and nothing outlives its last use).
        Product arithmetic of the frame-varying FIR, inference and training alike (the adjoint kernels work from the saved
        inputs in fp32 products): the context's mode (`hipddsp.Context.set_math`, default split-bf16), passed as
        `math=ctx.fir_math`; `ctx.ltv_fir` itself defaults to fp32 products."""
        raise NotImplementedError

    def _crop(self, ctx, n_dev, Fr):
        """`crop(*signals)`: zeroes (B, T) signals past every row's end in place (ragged; None entries are skipped) or does
        nothing.  A chain crops every signal before it enters the next filter; the crop is its own adjoint, so the chain's
        adjoint (`_train_backward`) crops the gradient at the same places."""
        return (lambda *xs: ctx.ragged_crop_(n_dev, Fr, self._hop, *xs)) if n_dev is not None else (lambda *xs: None)

    def _stages(self, ctx, n_dev, Fr, keep):
        """(crop, saved, save) of a chain: `crop` as `_crop` gives it; `save(tensors)` appends to `saved` in a training
        forward and drops them in inference, where an impulse-response matrix - the largest tensors of a forward - is
        released as soon as the next one replaces it."""
        saved = [] if keep else None
        return self._crop(ctx, n_dev, Fr), saved, (saved.extend if keep else (lambda xs: None))

    _GROUP_MIN_ROWS = 8192   # ddsp_fir_from_ctrl_group groups from here on

    def _filters(self, ctx, c2, problems, rows, f0_frames, keep):
        """Iterator over the filters of a chain, `problems` = [(mode, first column, n_mag)] in the order the chain uses them.
        Large inference batches: all of them from one grouped call (two launches) up front.  Training, which saves them one
        by one, and small batches, where the grouped call would run the single calls anyway: each when the chain asks for
        it, just before the FIR launch that reads it."""
        if keep or rows < self._GROUP_MIN_ROWS:
            return (ctx.fir_from_ctrl(mode, c2, col, n_mag, rows, self._sr, f0_frames if mode == FIR_DYNAMIC else None)
                    for mode, col, n_mag in problems)
        return iter(ctx.fir_from_ctrl_group(c2, problems, rows, self._sr, f0_frames))

    def _ragged_noise(self, ctx, n_dev, B, Fr, noise, noise_seed):
        """(unit-noise draw (B,T) with 0.5 - no excitation - past every row's end, EXC_UNIT_NOISE, 0)."""
        seed = 0 if noise is not None else (hipddsp.seed_from_torch() if noise_seed is None else int(noise_seed))
        return ctx.ragged_noise(noise, seed, n_dev, B, Fr, self._hop), EXC_UNIT_NOISE, 0

    @staticmethod
    def _noise_args(noise, noise_seed):
        if noise is not None:
            return noise.contiguous().float(), EXC_UNIT_NOISE, 0
        return None, EXC_GENERATE, (hipddsp.seed_from_torch() if noise_seed is None else int(noise_seed))

    def _phase_out(self, ctx, ps, n_dev=None):
        """The phase a forward returns - sample-rate where the model asks the scan for it (Sins), else frame-rate -, 0 over
        the padding of a ragged batch."""
        if self._front_wants.get("want_phase"):
            if n_dev is not None:
                ctx.ragged_crop_(n_dev, ps["phase_frames"].shape[1], self._hop, ps["phase"])
            return ps["phase"]
        pf = ps["phase_frames"]
        return pf if n_dev is None else ctx.ragged_frames(pf, n_dev, hold=False, out=pf)

    @staticmethod
    def _result(phase, outs):
        """(signal, phase (..., 1), (harmonic, noise)); a chain with one output (CombSubFast) returns it three times."""
        return outs[0], phase.unsqueeze(-1), tuple(outs[1:]) or (outs[0], outs[0])

    def _empty_result(self, f0_frames):
        """The result tuple of an empty batch (nothing is launched)."""
        Fr = f0_frames.shape[1]
        T = Fr * self._hop
        z = lambda n: torch.zeros(0, n, device=f0_frames.device)
        return self._result(z(T if self._front_wants.get("want_phase") else Fr), [z(T) for _ in range(self._n_outs)])

    @staticmethod
    def _mix_keyword(spk_mix_rows, kwargs):
        """`spk_mix_frames=(ids (B, K), w (B, Fr, K))` among a forward's extra keywords -> what `_forward` takes as
        `spk_mix_rows` (the per-frame form is that pair with a frame axis in w); ValueError with `spk_mix_rows` beside it."""
        frames = kwargs.get("spk_mix_frames")
        if frames is None:
            return spk_mix_rows
        if spk_mix_rows is not None:
            raise ValueError("spk_mix_frames= (a mix per frame) and spk_mix_rows= (a mix per row) are mutually exclusive")
        if not (isinstance(frames, (tuple, list)) and len(frames) == 2 and is_frame_mix(tuple(frames))):
            raise ValueError("spk_mix_frames must be a pair (ids (B, K) int32, w (B, Fr, K) fp32)")
        return tuple(frames)

    def _check_mix_rows(self, spk_mix_dict, spk_mix_rows, B):
        """`forward(..., spk_mix_rows=(ids, w))`: refusals before anything is launched (shapes and dtypes on the host;
        the ids of device tables are checked by the kernel that reads them, through the context's device error word)."""
        if spk_mix_dict is not None:
            raise ValueError("spk_mix_rows= (a mix per row, device tables) and spk_mix_dict (one host mix for the batch) are "
                             "mutually exclusive")
        if not (isinstance(spk_mix_rows, (tuple, list)) and len(spk_mix_rows) == 2):
            raise ValueError("spk_mix_rows must be a pair (ids (B, K) int32, w (B, K) fp32)")
        hipddsp.check_mix_rows(spk_mix_rows[0], spk_mix_rows[1], B, int(self.unit2ctrl.n_spk))
        if self.unit2ctrl.wants_grad():
            raise NotImplementedError("spk_mix_rows= is inference only: the training entries take spk_id or spk_mix_dict; call "
                                      "the model under torch.no_grad()")

    MAX_FORMANT = 24.0   # semitones, either way

    def _formant_segments(self):
        """[(first column, n, origin)] of the control row that a formant shift warps: origin 0 for magnitude bins, 1 for
        harmonics (`ddsp_ctrl_warp`)."""
        raise NotImplementedError

    def _warp(self, ctx, ctrl, formant, n_dev):
        """In place on the control matrix (B, Fr, sum): the formant shift, `formant` = (factors, slot_of_row | None)."""
        B, Fr = ctrl.shape[0], ctrl.shape[1]
        ctx.ctrl_warp_(ctrl.reshape(B * Fr, -1), self._formant_segments(), formant[0], Fr, slot_of_row=formant[1], n_dev=n_dev)

    def _formant_factors(self, formant, B, Fr, device):
        """`forward_formant`'s `formant` -> (factors fp32 device tensor, slot_of_row | None) or None (0 semitones: nothing to
        launch).  ValueError before anything is launched for a shift outside +-24 semitones or a tensor of another shape, dtype
        or device; the VALUES of a device tensor are the kernel's to check."""
        if isinstance(formant, (tuple, list)):
            if not (len(formant) == 2 and all(isinstance(t, torch.Tensor) for t in formant)):
                raise ValueError("formant: a pair is (factors (S,) fp32, slot_of_row (B,) int32), device tensors")
            factors, rows = formant
            if not (factors.dtype == torch.float32 and factors.dim() == 1 and factors.numel() >= 1 and rows.dtype == torch.int32 and
                    tuple(rows.shape) == (B,) and factors.device == rows.device == device):
                raise ValueError(f"formant: a pair is (factors (S,) fp32, slot_of_row (B = {B},) int32) on {device}")
            return factors.contiguous(), rows.contiguous()
        if isinstance(formant, torch.Tensor):
            if formant.dtype != torch.float32 or formant.device != device or tuple(formant.shape) not in ((B,), (B, Fr)):
                raise ValueError(f"formant: a tensor holds fp32 FACTORS on {device}, (B,) = ({B},) or (B, Fr) = ({B}, {Fr}); got "
                                 f"{formant.dtype} {tuple(formant.shape)} on {formant.device}")
            return formant.contiguous(), None
        factor = hipddsp.formant_factor(formant, self.MAX_FORMANT)
        if factor == 1.0:
            return None
        return torch.full((B,), factor, dtype=torch.float32, device=device), None

    def forward_formant(self, units_frames, f0_frames, volume_frames, spk_id, formant, spk_mix_dict=None, initial_phase=None,
                        infer=True, noise=None, noise_seed=None, n_frames=None, spk_mix_rows=None):
        """`forward` with a formant shift (module docstring): `formant` semitones (a number, |s| <= 24) or fp32 device FACTORS
        (B,) / (B, Fr) / (factors (S,), slot_of_row (B,) int32); returns `forward`'s tuple.  Inference only."""
        if self.unit2ctrl.wants_grad():
            raise NotImplementedError("formant= is inference only: the warp has no adjoint; call the model under torch.no_grad()")
        B, Fr = units_frames.shape[0], units_frames.shape[1]
        return self._forward(units_frames, f0_frames, volume_frames, spk_id, spk_mix_dict, initial_phase, infer, noise,
                             noise_seed, n_frames, spk_mix_rows, formant=self._formant_factors(formant, B, Fr, f0_frames.device))

    def _forward(self, units_frames, f0_frames, volume_frames, spk_id, spk_mix_dict, initial_phase, infer, noise,
                 noise_seed, n_frames, spk_mix_rows, formant=None):
        """The body of every model's `forward`.  Launches, in order: [ragged: the counts' upload and the held form of units,
        f0 and volume;] the phase scan; the control network; [`formant`: the warp;] the model's chain; [ragged: the padding of
        the returned phase cleared].  A call that autograd records is the same sequence inside `_SynthTrainFn.forward`.
        `formant`: None or `_formant_factors`' (factors, slot_of_row | None).  Ragged, the warp sits between the control network
        and the hold of its last frame over the padding: the kernel leaves the frames past a row's count alone, and the hold
        then gives the chain the held form of the WARPED matrix."""
        B, Fr = units_frames.shape[0], units_frames.shape[1]
        spk_mix_dict, spk_mix_rows = self.unit2ctrl.frame_mix(spk_mix_dict, spk_mix_rows, B, Fr, units_frames.device)
        if spk_mix_rows is not None and not is_frame_mix(spk_mix_rows):
            self._check_mix_rows(spk_mix_dict, spk_mix_rows, B)
        if B == 0:
            return self._empty_result(f0_frames)
        vals = None if n_frames is None else self.unit2ctrl.check_ragged(n_frames, B, Fr)
        if vals is not None and not self.training and self.unit2ctrl.wants_grad():
            raise NotImplementedError("n_frames= (ragged batches) on a model in eval mode is inference only: call the model "
                                      "under torch.no_grad(), or put it into training mode (model.train()) to have the ragged "
                                      "call recorded for autograd")
        if formant is not None and self.unit2ctrl.wants_grad():
            raise NotImplementedError("formant= is inference only: the warp has no adjoint; call the model under torch.no_grad()")
        if self.unit2ctrl.wants_grad():
            phase, *outs = _SynthTrainFn.apply(self, units_frames, f0_frames, volume_frames, spk_id, spk_mix_dict,
                                               initial_phase, infer, noise, noise_seed, vals, *self.unit2ctrl.parameters())
            return self._result(phase, outs)
        if vals is not None:
            ctx = self._context(f0_frames, ragged=True)
            n_dev, units, f0, _, volume = self.unit2ctrl.hold_ragged(ctx, vals, units_frames, f0_frames, None, volume_frames)
            f0 = f0.reshape(B, Fr, 1)
            ps = self._scan(ctx, f0, initial_phase, infer)
            ctrl = self.unit2ctrl.forward_ragged(ctx, units, f0, ps["phase_frames"], volume, spk_id, spk_mix_dict, n_dev,
                                                 hold=formant is None,
                                                 spk_mix_rows=self.unit2ctrl.hold_frame_mix(ctx, spk_mix_rows, n_dev))
            if formant is not None:
                self._warp(ctx, ctrl, formant, n_dev)
                ctx.ragged_frames(ctrl, n_dev, hold=True, out=ctrl)
            excitation = lambda: self._ragged_noise(ctx, n_dev, B, Fr, noise, noise_seed)
        else:
            n_dev, f0 = None, f0_frames
            ctx = self._context(f0)
            ps = self._scan(ctx, f0, initial_phase, infer)
            ctrl = self.unit2ctrl.forward_flat(units_frames, f0, ps["phase_frames"], volume_frames, spk_id, spk_mix_dict,
                                               spk_mix_rows=spk_mix_rows)
            if formant is not None:
                self._warp(ctx, ctrl, formant, None)
            excitation = lambda: self._noise_args(noise, noise_seed)
        outs, _ = self._render(ctx, ctrl, ps, f0, excitation, n_dev)
        return self._result(self._phase_out(ctx, ps, n_dev), outs)


class _SynthTrainFn(torch.autograd.Function):
    """Autograd node of one synthesiser forward: forward and backward are libddsp_amd calls end to end; torch only
    routes the parameter gradients (reference: autograd through `*.forward`, solver.py:111-113).  The model supplies
    `_render(ctx, ctrl, ps, f0_frames, excitation, n_dev, keep=True) -> (outputs, saved)` and
    `_train_backward(ctx, ctrl, saved, f0_frames, noise_args, grads, crop) -> d_ctrl (rows, sum)`.
    `vals`: the checked counts of a ragged batch or None.  Ragged, the forward is the ragged inference forward with its
    activations kept (held inputs, the control matrix held over the padding, the noise draw of `_ragged_noise`, every
    signal cropped), and the backward its adjoint: the upstream gradients are cropped to the rows, the chain's adjoint crops
    where the chain cropped, the adjoint of the hold folds the padding frames of d_ctrl into each row's last frame, and
    the control network's backward takes the counts."""

    @staticmethod
    def forward(fctx, model, units, f0_frames, volume, spk_id, spk_mix_dict, initial_phase, infer, noise, noise_seed, vals,
                *params):
        ctx = model._context(f0_frames, ragged=vals is not None)
        B, Fr = units.shape[0], units.shape[1]
        n_dev = None
        if vals is not None:
            n_dev, units, f0, _, volume = model.unit2ctrl.hold_ragged(ctx, vals, units, f0_frames, None, volume)
            f0_frames = f0.reshape(B, Fr, 1)
        ps = model._scan(ctx, f0_frames, initial_phase, infer)
        # the training forward runs fp32 products throughout (control network, filter synthesis, FIR): the loss gradient
        # amplifies a 4e-6 error of the signal a thousandfold (tools/diag_train_b32.py).  The BACKWARD runs on the
        # context's own mode: its weight / input gradient GEMMs use split-bf16 products by default (a 4e-6 product error
        # inside the backward is not amplified); `ctx.set_math(MATH_FP32)` around `loss.backward()` makes them fp32 too
        keep_math = ctx.math
        ctx.set_math(hipddsp.MATH_FP32)
        try:
            if n_dev is None:
                ctrl, kept = model.unit2ctrl.forward_flat_keep(units, f0_frames, ps["phase_frames"], volume, spk_id,
                                                               spk_mix_dict, ctx=ctx)
                nargs = model._noise_args(noise, noise_seed)
            else:
                ctrl, kept = model.unit2ctrl.forward_ragged_keep(ctx, units, f0_frames, ps["phase_frames"], volume, spk_id,
                                                                 spk_mix_dict, n_dev)
                nargs = model._ragged_noise(ctx, n_dev, B, Fr, noise, noise_seed)
            outs, saved = model._render(ctx, ctrl, ps, f0_frames, lambda: nargs, n_dev, keep=True)
        finally:
            ctx.set_math(keep_math)
        fctx.model, fctx.dsp = model, ctx
        fctx.set_materialize_grads(False)   # outputs the loss does not use arrive as None in backward, not as zero tensors to add
        fctx.args = (units, f0_frames, volume, spk_id, spk_mix_dict, nargs, ps["phase_frames"], n_dev)
        fctx.saved = (ctrl, saved, kept)
        phase_out = model._phase_out(ctx, ps, n_dev)
        fctx.mark_non_differentiable(phase_out)
        return (phase_out,) + tuple(outs)

    @staticmethod
    def backward(fctx, d_phase, *d_outs):
        model, ctx = fctx.model, fctx.dsp
        units, f0_frames, volume, spk_id, spk_mix_dict, nargs, phase_frames, n_dev = fctx.args
        if fctx.saved is None:
            raise RuntimeError("this synthesiser forward was already back-propagated (its kept activations are released)")
        ctrl, saved, kept = fctx.saved
        B, Fr = ctrl.shape[0], ctrl.shape[1]
        crop = model._crop(ctx, n_dev, Fr)
        if n_dev is not None:   # (copies: the upstream gradients are autograd's)
            d_outs = tuple(None if g is None else g.float().contiguous().clone() for g in d_outs)
            crop(*d_outs)
        d_ctrl = model._train_backward(ctx, ctrl, saved, f0_frames, nargs, d_outs, crop).reshape(B, Fr, -1)
        if n_dev is not None:
            ctx.ragged_frames_adjoint_(d_ctrl, n_dev)
        grads = model.unit2ctrl.backward_flat(units, f0_frames, phase_frames, volume, spk_id, spk_mix_dict, d_ctrl, ctx=ctx,
                                              kept=kept, n_dev=n_dev)
        fctx.saved = None
        params = tuple(grads.get(p) for p in model.unit2ctrl.parameters())
        return (None,) * (len(fctx.needs_input_grad) - len(params)) + params      # no gradient for what precedes *params


def _sum_grads(ref, *gs):
    """Sum of the upstream gradients that exist (zeros when none does)."""
    acc = None
    for g in gs:
        if g is not None:
            acc = g.contiguous() if acc is None else acc + g
    return torch.zeros_like(ref) if acc is None else acc


class CombSub(_SynthBase):
    """Combtooth subtractive synthesiser, classic variant (reference `ddsp/vocoder.py:495-550`)."""

    def __init__(self, sampling_rate, block_size, n_mag_allpass, n_mag_harmonic, n_mag_noise, n_unit=256, n_spk=1,
                 c=False):
        super().__init__(sampling_rate, block_size)
        print(" [DDSP Model] Combtooth Subtractive Synthesiser (Old Version)")
        self.n_mags = (int(n_mag_allpass), int(n_mag_harmonic), int(n_mag_noise))
        self.unit2ctrl = Unit2Control(n_unit, n_spk, {"group_delay": n_mag_allpass,
                                                      "harmonic_magnitude": n_mag_harmonic,
                                                      "noise_magnitude": n_mag_noise}, c)

    _comb_mode = COMB_SINC
    _front_wants = {}
    _n_outs = 3

    def _formant_segments(self):
        na, nh, nn_ = self.n_mags
        return [(na, nh, 0), (na + nh, nn_, 0)]                  # harmonic_magnitude, noise_magnitude; group_delay stays

    def _render(self, ctx, ctrl, ps, f0_frames, excitation, n_dev=None, keep=False):
        """Combtooth -> all-pass -> harmonic filter, + filtered noise -> ((signal, harmonic, noise), saved).  Ragged: the
        all-pass output is cropped too, as the reference crops per call."""
        B, Fr = ctrl.shape[0], ctrl.shape[1]
        rows, sr, hop = B * Fr, self._sr, self._hop
        na, nh, nn_ = self.n_mags
        c2 = ctrl.reshape(rows, -1)
        crop, saved, save = self._stages(ctx, n_dev, Fr, keep)
        comb = ps["comb"]
        crop(comb)
        firs = self._filters(ctx, c2, [(FIR_ALLPASS, 0, na), (FIR_DYNAMIC, na, nh), (FIR_STATIC, na + nh, nn_)], rows,
                             f0_frames, keep)
        ir = next(firs)
        h, _ = ctx.ltv_fir(comb, ir, B, Fr, hop, math=ctx.fir_math)
        crop(h)
        save((comb, h, ir))
        ir = next(firs)
        harmonic, _ = ctx.ltv_fir(h, ir, B, Fr, hop, math=ctx.fir_math)
        crop(harmonic)
        save((ir,))
        ir = next(firs)
        nz, exc, seed = excitation()
        noise_out, signal = ctx.ltv_fir(nz, ir, B, Fr, hop, excitation=exc, noise_seed=seed, add_in=harmonic,
                                        math=ctx.fir_math)
        crop(noise_out, signal)
        save((ir,))
        return (signal, harmonic, noise_out), saved

    def _train_backward(self, ctx, ctrl, saved, f0_frames, nargs, d_outs, crop):
        comb, h1, ir_ap, ir_h, ir_n = saved
        d_signal, d_harm, d_noise = d_outs
        B, Fr = ctrl.shape[0], ctrl.shape[1]
        rows, sr, hop = B * Fr, self._sr, self._hop
        na, nh, nn_ = self.n_mags
        nz, exc, seed = nargs
        d_h = _sum_grads(comb, d_signal, d_harm)
        d_n = _sum_grads(comb, d_signal, d_noise)
        c2 = ctrl.reshape(rows, -1)
        d_ctrl = torch.empty_like(c2)
        _, d_ir = ctx.ltv_fir_bwd(nz, ir_n, d_n, B, Fr, hop, excitation=exc, noise_seed=seed, want_d_audio=False)
        ctx.fir_from_ctrl_bwd(FIR_STATIC, c2, na + nh, nn_, rows, sr, d_ir, d_ctrl)
        d_h1, d_ir = ctx.ltv_fir_bwd(h1, ir_h, d_h, B, Fr, hop)
        crop(d_h1)
        ctx.fir_from_ctrl_bwd(FIR_DYNAMIC, c2, na, nh, rows, sr, d_ir, d_ctrl, f0_frames)
        _, d_ir = ctx.ltv_fir_bwd(comb, ir_ap, d_h1, B, Fr, hop, want_d_audio=False)
        ctx.fir_from_ctrl_bwd(FIR_ALLPASS, c2, 0, na, rows, sr, d_ir, d_ctrl)
        return d_ctrl

    def forward(self, units_frames, f0_frames, volume_frames, spk_id, spk_mix_dict=None, initial_phase=None,
                infer=True, noise=None, noise_seed=None, n_frames=None, spk_mix_rows=None, **kwargs):
        """units (B,Fr,n_unit), f0 (B,Fr,1) Hz, volume (B,Fr), spk_id (B,1)|(1,1) int64 1-based ->
        (signal (B,T), phase_frames (B,Fr,1), (harmonic (B,T), noise (B,T))).  `n_frames`: ragged batch,
        `spk_mix_rows`: a speaker mix per row, `spk_mix_frames=`: one per frame (module docstring)."""
        return self._forward(units_frames, f0_frames, volume_frames, spk_id, spk_mix_dict, initial_phase, infer, noise,
                             noise_seed, n_frames, self._mix_keyword(spk_mix_rows, kwargs))


class Sins(_SynthBase):
    """Sinusoids additive synthesiser (reference `ddsp/vocoder.py:372-423`)."""

    def __init__(self, sampling_rate, block_size, n_harmonics, n_mag_allpass, n_mag_noise, n_unit=256, n_spk=1,
                 c=False):
        super().__init__(sampling_rate, block_size)
        print(" [DDSP Model] Sinusoids Additive Synthesiser")
        self.n_mags = (int(n_harmonics), int(n_mag_allpass), int(n_mag_noise))
        self.unit2ctrl = Unit2Control(n_unit, n_spk, {"amplitudes": n_harmonics, "group_delay": n_mag_allpass,
                                                      "noise_magnitude": n_mag_noise}, c)

    _comb_mode = COMB_NONE
    _front_wants = {"want_phase": True}
    _n_outs = 3

    def _formant_segments(self):
        nhm, na, nn_ = self.n_mags
        return [(0, nhm, 1), (nhm + na, nn_, 0)]                 # amplitudes (harmonic j + 1), noise_magnitude; group_delay stays

    def _render(self, ctx, ctrl, ps, f0_frames, excitation, n_dev=None, keep=False):
        """Sinusoid bank on the sample-rate phase -> all-pass, + filtered noise -> ((signal, harmonic, noise), saved)."""
        B, Fr = ctrl.shape[0], ctrl.shape[1]
        rows, sr, hop = B * Fr, self._sr, self._hop
        nhm, na, nn_ = self.n_mags
        c2 = ctrl.reshape(rows, -1)
        crop, saved, save = self._stages(ctx, n_dev, Fr, keep)
        sinusoids = ctx.sins_bank(c2, 0, nhm, f0_frames, ps["phase"], B, Fr, hop, sr)
        crop(sinusoids)
        firs = self._filters(ctx, c2, [(FIR_ALLPASS, nhm, na), (FIR_STATIC, nhm + na, nn_)], rows, f0_frames, keep)
        ir = next(firs)
        harmonic, _ = ctx.ltv_fir(sinusoids, ir, B, Fr, hop, math=ctx.fir_math)
        crop(harmonic)
        save((ps["phase"], sinusoids, ir))
        ir = next(firs)
        nz, exc, seed = excitation()
        noise_out, signal = ctx.ltv_fir(nz, ir, B, Fr, hop, excitation=exc, noise_seed=seed, add_in=harmonic,
                                        math=ctx.fir_math)
        crop(noise_out, signal)
        save((ir,))
        return (signal, harmonic, noise_out), saved

    def _train_backward(self, ctx, ctrl, saved, f0_frames, nargs, d_outs, crop):
        phase, sinusoids, ir_ap, ir_n = saved
        d_signal, d_harm, d_noise = d_outs
        B, Fr = ctrl.shape[0], ctrl.shape[1]
        rows, sr, hop = B * Fr, self._sr, self._hop
        nhm, na, nn_ = self.n_mags
        nz, exc, seed = nargs
        d_h = _sum_grads(sinusoids, d_signal, d_harm)
        d_n = _sum_grads(sinusoids, d_signal, d_noise)
        c2 = ctrl.reshape(rows, -1)
        d_ctrl = torch.empty_like(c2)
        _, d_ir = ctx.ltv_fir_bwd(nz, ir_n, d_n, B, Fr, hop, excitation=exc, noise_seed=seed, want_d_audio=False)
        ctx.fir_from_ctrl_bwd(FIR_STATIC, c2, nhm + na, nn_, rows, sr, d_ir, d_ctrl)
        d_sin, d_ir = ctx.ltv_fir_bwd(sinusoids, ir_ap, d_h, B, Fr, hop)
        crop(d_sin)
        ctx.fir_from_ctrl_bwd(FIR_ALLPASS, c2, nhm, na, rows, sr, d_ir, d_ctrl)
        ctx.sins_bank_bwd(c2, 0, nhm, f0_frames, phase, d_sin, B, Fr, hop, sr, d_ctrl)
        return d_ctrl

    def forward(self, units_frames, f0_frames, volume_frames, spk_id, spk_mix_dict=None, initial_phase=None,
                infer=True, max_upsample_dim=32, noise=None, noise_seed=None, n_frames=None, spk_mix_rows=None):
        """Same contract as CombSub.forward except that the returned phase is sample-rate (B,T,1)
        (reference `ddsp/vocoder.py:423`).  `max_upsample_dim` is accepted and ignored: the bank kernel never
        materialises the (B,T,chunk) tensors the reference chunks to bound."""
        return self._forward(units_frames, f0_frames, volume_frames, spk_id, spk_mix_dict, initial_phase, infer, noise,
                             noise_seed, n_frames, spk_mix_rows)


class CombSubFast(_SynthBase):
    """Combtooth subtractive synthesiser, windowed spectral OLA variant (reference `ddsp/vocoder.py:426-492`)."""

    def __init__(self, sampling_rate, block_size, n_unit=256, n_spk=1, c=False):
        super().__init__(sampling_rate, block_size)
        print(" [DDSP Model] Combtooth Subtractive Synthesiser")
        self.register_buffer("window", torch.sqrt(torch.hann_window(2 * block_size)))
        nb = int(block_size) + 1
        self.unit2ctrl = Unit2Control(n_unit, n_spk, {"harmonic_magnitude": nb, "harmonic_phase": nb,
                                                      "noise_magnitude": nb}, c)

    _comb_mode = COMB_SINC_GATED
    _front_wants = {}
    _n_outs = 1

    def _formant_segments(self):
        nb = self._hop + 1
        return [(0, nb, 0), (2 * nb, nb, 0)]                     # harmonic_magnitude, noise_magnitude; harmonic_phase stays

    def _render(self, ctx, ctrl, ps, f0_frames, excitation, n_dev=None, keep=False):
        """One windowed spectral OLA -> ((signal,), saved).  Ragged: with the comb and the excitation 0 past a row's end,
        frames 0..n_b of the row are the frames of the row rendered alone (frame n_b on frame n_b - 1's filters, `block_size`
        zeros behind the row)."""
        B, Fr = ctrl.shape[0], ctrl.shape[1]
        crop, saved, save = self._stages(ctx, n_dev, Fr, keep)
        comb = ps["comb"]
        crop(comb)
        nz, exc, seed = excitation()
        signal = ctx.spectral_ola(ctrl.reshape(B * Fr, -1), comb, nz, exc, seed, B, Fr, self._hop)
        crop(signal)
        save((comb,))
        return (signal,), saved

    def _train_backward(self, ctx, ctrl, saved, f0_frames, nargs, d_outs, crop):
        (comb,) = saved
        B, Fr = ctrl.shape[0], ctrl.shape[1]
        nz, exc, seed = nargs
        return ctx.spectral_ola_bwd(ctrl.reshape(B * Fr, -1), comb, nz, exc, seed, _sum_grads(comb, *d_outs), B, Fr,
                                    self._hop)

    def forward(self, units_frames, f0_frames, volume_frames, spk_id, spk_mix_dict=None, initial_phase=None,
                infer=True, noise=None, noise_seed=None, n_frames=None, spk_mix_rows=None, **kwargs):
        """Returns (signal, phase_frames (B,Fr,1), (signal, signal)) - the same tensor three times, like the
        reference (`ddsp/vocoder.py:492`).  `n_frames`: ragged batch,
        `spk_mix_rows`: a speaker mix per row, `spk_mix_frames=`: one per frame (module docstring)."""
        return self._forward(units_frames, f0_frames, volume_frames, spk_id, spk_mix_dict, initial_phase, infer, noise,
                             noise_seed, n_frames, self._mix_keyword(spk_mix_rows, kwargs))
