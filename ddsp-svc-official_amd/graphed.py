"""HIP-graph replay of the real-time forwards for one fixed shape: the synthesiser alone (`GraphedSynth`), the whole block from
the raw audio on (`GraphedBlock`), one model's rows of a bank with a model per slot (`GraphedModelRows`) and the enhancer stage
of a bank (`GraphedBankEnhancer`).

The real-time caller (`gui.py:360-430`: one 0.2 s block at a time, B = 1, 87 frames) is launch-bound: ~50 kernels of
a few microseconds each, paced by Python + ctypes + hipLaunch on the host.  A capture records the whole call once
(`torch.cuda.graph`: stream capture also records the kernels libddsp_amd launches on that stream) and replays it with one
host call per block.

What makes the capture safe is one protocol, `_Captured._capture`, that all these classes go through; its ORDER is the rule:
  1. the captured library calls go through a `hipddsp.Context` of their own (`hipddsp.use_context`): the captured kernels
     point into THAT context's scratch arena, tables and zero page;
  2. those are sized by eager warm-up runs of `_run()` on a side stream (after a `wait_stream` on the caller's, and waited for
     and synchronised afterwards): first-use allocations, tap tables and the analysis networks' prepared weights happen here;
  3. `_run()` is captured, on one stream (a linear graph);
  4. the context is frozen (`Context.freeze`): no later eager call can regrow or reuse what the graph points into;
  5. caller tensors that `_run()` changes in place (the window(s)) are cloned before step 2 and copied back after step 4, so a
     re-capture in the middle of a stream keeps the stream; only then is a dither seed drawn.
Further rules:
  * random inputs (the noise excitation, the enhancer's source phases) come from static device tensors that are refilled
    before every replay (`_refill`; the eager path draws a host seed per call, which a graph would freeze);
  * inputs are copied into static tensors, outputs are static tensors valid until the next replay.
Weights are read by the captured kernels at replay time (the weight-preparation kernel is part of the graph), so
in-place weight updates are honoured.  `spk_mix_dict` ({speaker id: weight}) is captured with the graph: its ids and
weights become kernel arguments, so a capture is valid for that mix only (a new mix needs a new capture;
`realtime.StreamRenderer.set_speaker` does that), while `spk_id` stays a static input.  With `spk_mix_rows=True` (or a K) the
speaker term is a mix per row held in two static device tables, `mix_ids` (B, K) int32 and `mix_w` (B, K) fp32
(`forward(..., spk_mix_rows=)`): the captured kernels read them at replay time, so any row's speaker or mix changes by a write to
its table row, without a new capture.  `initial_phase` is a host-side argument and not supported here.  Forward only.

`GraphedBlock` captures the real-time block from the raw audio on (`block_chain`: window push, volume, f0 extractor, pitch
shift, units encoder, synthesiser, volume gate) under the same rules.  It takes one window (n_in,) - the solo kernels, a host
pitch factor, `spk_id` static and `spk_mix_dict` captured (`realtime.StreamRenderer`) - or S windows (S, n_in) of one geometry -
the batch kernels, with the speaker mix and the pitch factor of every row as device data (`realtime.StreamBank`).  Three
networks then share the captured context; each has a prepared-weight slot of its own in it.  The control network's weights are
prepared inside the graph on every replay (in-place updates are honoured, as above); the two analysis networks (HuBERT-Soft,
CREPE: inference only) are prepared once by the warm-up runs and the captured kernels read those copies
(`ddsp_weight_slot_take(..., keep_in_capture)`), so a change of THEIR weights needs a new capture.  The CREPE dither seed lives
in a device word that the decode advances (`seed_dev` of `ddsp_crepe_decode`): a seed passed by value would be frozen by the capture.

`GraphedBankEnhancer` captures the enhancer stage of a `realtime.StreamBank` (`bank_enhancer_chain`: the per-row adaptive key
decided on the device, the keyed resamplers, the ragged generator, the resampling to the device rate and the gather of every
row's own tail) as a second linear graph that is replayed right after the first.  That it can be captured at all is the proof
that nothing in the stage asks the host: a row whose pitch crosses a key boundary changes device data, not the graph.
"""
import gc

import torch

import hipddsp


class _Captured:
    """The capture protocol of the module docstring.  A subclass builds its static tensors, then calls `_capture`, which
    leaves `self.ctx` and `self.graph` and returns what the captured `_run()` returned (the static outputs)."""

    def _capture(self, dev, warmup, keep=()):
        """`keep`: the caller's tensors that `_run()` changes in place; they are left as they were found."""
        self.ctx = hipddsp.Context(dev)
        kept = [t.clone() for t in keep]
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side), hipddsp.use_context(self.ctx), torch.no_grad():
            for _ in range(max(1, warmup)):   # arena, tap tables and the analysis networks' prepared weights: here, eagerly
                self._run()
        cur.wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        # The cyclic collector stays off while the stream captures: a dead cycle that holds an older capture (a bank and its
        # rows) would otherwise be collected whenever `_run()` allocates, and destroying a graph synchronises the device, which
        # a capturing stream refuses - from a destructor, that ends the process.
        collecting = gc.isenabled()
        gc.disable()
        try:
            with hipddsp.use_context(self.ctx), torch.no_grad(), torch.cuda.graph(self.graph):
                out = self._run()
        finally:
            if collecting:
                gc.enable()
        self.ctx.freeze()
        for t, k in zip(keep, kept):
            t.copy_(k)
        return out


def _refill(static, value):
    """A static random input before a replay: a fresh uniform draw, or the caller's `value` (parity tests)."""
    if value is None:
        static.uniform_()
    else:
        static.copy_(value)


class GraphedSynth(_Captured):
    def __init__(self, model, B, Fr, warmup=3, spk_mix_dict=None, spk_mix_rows=None, capture=True, formant=None):
        """`formant`: None, or the caller's device factors as `forward_formant` takes them - (B,) fp32, or the pair (factors (S,),
        slot_of_row (B,) int32) -, read by the captured warp at their fixed addresses (`realtime.StreamBank(formant=True)`).
        `spk_mix_rows`: None / False; True (K = 4 slots per row) or a K for static mix tables of the graph's own; or the
        caller's device tables (ids (B, K) int32, w (B, K) fp32), which the graph then reads at their fixed addresses; with
        w (B, Fr, K) they are a mix per FRAME (`hipddsp.check_mix_frames`), which reaches the control network's framemix entry.
        `capture=False` (a subclass that also runs eagerly, `GraphedModelRows`): the static tensors alone, `graph` is None."""
        rows = spk_mix_rows is not None and spk_mix_rows is not False
        if rows and spk_mix_dict is not None:
            raise ValueError("GraphedSynth: spk_mix_rows and spk_mix_dict are mutually exclusive")
        tables = spk_mix_rows if isinstance(spk_mix_rows, (tuple, list)) else None
        if tables is not None and isinstance(tables[1], torch.Tensor) and tables[1].dim() == 3:
            K = hipddsp.check_mix_frames(tables[0], tables[1], B, Fr)   # a mix per FRAME: w (B, Fr, K)
        elif tables is not None:
            K = hipddsp.check_mix_rows(tables[0], tables[1], B, int(model.unit2ctrl.n_spk))
        else:
            K = 0 if not rows else (4 if spk_mix_rows is True else int(spk_mix_rows))
            if rows and not 1 <= K <= hipddsp.MAX_MIX:
                raise ValueError(f"GraphedSynth: 1 to {hipddsp.MAX_MIX} slots per mix row, got {K}")
        p = next(model.parameters())
        if capture and not p.is_cuda:
            raise RuntimeError("GraphedSynth needs the model on a HIP device (no CPU fallback)")
        self.model = model.eval()
        self.device = p.device
        self.B, self.Fr = int(B), int(Fr)
        self.spk_mix_dict = None if spk_mix_dict is None else dict(spk_mix_dict)
        hop = int(model.block_size)
        n_unit = model.unit2ctrl.n_unit
        dev = self.device
        self.units = torch.zeros(B, Fr, n_unit, device=dev)
        self.f0 = torch.full((B, Fr, 1), 220.0, device=dev)
        self.volume = torch.zeros(B, Fr, device=dev)
        self.spk_id = torch.ones(B, 1, dtype=torch.int64, device=dev)
        self.noise = torch.rand(B, Fr * hop, device=dev)
        # the row mixes (speaker 1 with weight 1 in slot 0, padding behind it, until the caller writes the rows)
        if tables is not None:
            self.mix_ids, self.mix_w = tables
        else:
            self.mix_ids = torch.ones(B, K, dtype=torch.int32, device=dev) if K else None
            self.mix_w = torch.zeros(B, K, device=dev) if K else None
            if K:
                self.mix_w[:, 0] = 1.0
        self.formant = formant
        self.graph = None
        self.out = self._capture(dev, warmup) if capture else None

    def _run(self):
        if self.formant is not None:
            return self.model.forward_formant(self.units, self.f0, self.volume, self.spk_id, self.formant, noise=self.noise,
                                              **({"spk_mix_dict": self.spk_mix_dict} if self.mix_ids is None else
                                                 {"spk_mix_rows": (self.mix_ids, self.mix_w)}))
        if self.mix_ids is not None:
            return self.model(self.units, self.f0, self.volume, self.spk_id, spk_mix_rows=(self.mix_ids, self.mix_w),
                              noise=self.noise)
        return self.model(self.units, self.f0, self.volume, self.spk_id, spk_mix_dict=self.spk_mix_dict, noise=self.noise)

    @torch.no_grad()
    def __call__(self, units, f0, volume, spk_id, noise=None):
        """Same positional inputs as `model.forward`; returns the model's result tuple (static tensors, overwritten by
        the next call).  `noise` (B, T) in [0, 1) replaces the fresh uniform draw (parity tests).  With row mixes `spk_id` may
        be None (the tables `mix_ids` / `mix_w` carry the speakers)."""
        if tuple(units.shape[:2]) != (self.B, self.Fr):
            raise ValueError(f"GraphedSynth captured for (B, Fr) = {(self.B, self.Fr)}, got {tuple(units.shape[:2])}")
        self.units.copy_(units)
        self.f0.copy_(f0.reshape(self.f0.shape))
        self.volume.copy_(volume.reshape(self.volume.shape))
        if spk_id is not None:
            self.spk_id.copy_(spk_id.expand_as(self.spk_id) if spk_id.shape[0] == 1 else spk_id.reshape(self.spk_id.shape))
        _refill(self.noise, noise)
        self.graph.replay()
        return self.out


class GraphedModelRows(GraphedSynth):
    """The compact synthesis chain of ONE model of a `realtime.StreamBank(models=...)` at one width W: `GraphedSynth`'s static
    tensors and forward (with a mix per row) between the two row movers of csrc/bank_rows.hip.  `_run()` gathers the features
    of this model's rows out of the call's row batch (`ddsp_bank_features_gather`), runs the model, gates the signal with the
    gathered volume and scatters every real row into the call's signal (`ddsp_bank_signal_scatter`).
    `batch`: the bank's staging tensors of the call's rows, {"units" (R, Fr, C), "f0" (R, Fr, 1), "volume" (R, Fr), "noise"
    (R, Fr * block_size), "mix": (ids (R, K) int32, w (R, K))}, and `sig` (R, Fr * block_size), all the caller's and read or
    written at their fixed addresses.  `table` (W,) int32 is this chain's device row table: entry r the row of the batch behind
    compact row r, -1 for padding (zero units, f0 0, volume 0, speaker 1 with weight 1; computed, never scattered).  It is all
    padding while the capture runs, so a capture writes nothing of `sig`.  A call uploads the table only when it differs from the
    one on the device.  `replays` counts the calls.  With `capture=False` the same `_run()` runs eagerly."""

    def __init__(self, model, W, Fr, batch, sig, threshold_db, warmup=3, capture=True):
        self.batch, self.sig, self.threshold_db = batch, sig, float(threshold_db)
        self.hop = int(model.block_size)                             # (a host int before the capture: no read-back inside it)
        self.table = torch.full((int(W),), -1, dtype=torch.int32, device=sig.device)
        self.named = ()                                              # the real rows of `table`, as the host knows them
        self.replays = 0
        super().__init__(model, W, Fr, warmup=warmup, spk_mix_rows=int(batch["mix"][0].shape[1]), capture=capture)

    def _run(self):
        ctx, b = hipddsp.context_for(self.device), self.batch       # (under capture: the captured context, `use_context`)
        ctx.bank_features_gather_(self.table, b["units"], b["f0"], b["volume"], b["mix"], self.units, self.f0, self.volume,
                                  (self.mix_ids, self.mix_w), b["noise"], self.noise)
        out = super()._run()
        ctx.volume_gate_(out[0], self.volume, self.threshold_db, self.hop)
        ctx.bank_signal_scatter_(self.table, out[0], self.sig)
        return out

    @torch.no_grad()
    def __call__(self, named):
        """`named`: the rows of the batch that this model renders, 1 to W ints in [0, R), no row twice."""
        named = tuple(named)
        if not 1 <= len(named) <= self.B:
            raise ValueError(f"GraphedModelRows captured for {self.B} rows, got {len(named)}")
        if named != self.named:
            self.table.copy_(torch.tensor(list(named) + [-1] * (self.B - len(named)), dtype=torch.int32))
            self.named = named
        self.replays += 1
        if self.graph is not None:
            self.graph.replay()
        else:
            self._run()


def block_chain(ctx, model, units_encoder, f0_extractor, window, block_in, samplerate, hop_size, silence_front, pitch,
                threshold_db, block_size, speaker, noise=None, f0_dither=True, seed_dev=None, push=None, envelope=None,
                tune=None, retrieve=None):
    """One block of the reference's callback from the raw audio to the gated model output (gui.py:373-374 and
    `gui.SvcDDSP.infer`, gui.py:87-127), every step on the device, nothing read back: `window` takes `block_in` in place,
    then volume, f0 (uv_interp, silent front), the pitch shift, units, the synthesiser and the gate.
    One stream: `window` (n_in,), `block_in` (block,), `pitch` a host factor (no multiply at exactly 1).  S streams of one
    geometry: `window` (S, n_in), `block_in` (S, block), `pitch` a device (S,) tensor of factors - or (S, Fr), a factor per FRAME,
    which `push` fills (`ddsp_bank_key_glide`) -; every step is then one batched call.  The window keeps the rank it comes with down to the library, so each form reaches its own kernels.
    `speaker`: the speaker term as the model's keyword arguments - with a "formant" among them (`forward_formant`'s device
    factors) the synthesiser is entered through `forward_formant` -, {"spk_id": (1, 1) int64, "spk_mix_dict": dict or None} or
    {"spk_id": None, "spk_mix_rows": (ids (S, K) int32, w (S, K) fp32)}.
    `push(ctx, window, block_in)`: the step that brings `window` up to date, `ctx.stream_push_` unless given.  The compact rows of
    a bank's active set (`realtime.StreamBank`, `active=`) are the S-stream form with `Context.bank_gather_` as this step: it pushes
    the blocks into the named slots' own windows and fills `window`, `pitch` and the mix tables (the compact ones) from them.
    `model=None` stops after the features: the signal is None, and the synthesis and the gate are the caller's (a bank with a
    model per slot renders every model's rows on their own, `GraphedModelRows`); `speaker`, `noise` and `block_size` are unused.
    `tune`: None, or the pitch correction of the rows as device tensors (mask (S,) int32, param (S, 3) fp64, slot_of_row (rows,)
    int32 or None: row b is slot b): one `Context.f0_tune_` right behind the pitch multiply, so units, the synthesiser and whoever
    takes the returned f0 (an enhancer) see the corrected one.
    `retrieve`: None, or the unit retrieval of the rows (bank - an `infer_offline.UnitIndexBank` -, index_of_slot (S,) int32,
    ratio_of_slot (S,) fp32, k, slot_of_row (rows,) int32 or None: row b is slot b): one `Context.units_retrieve_` right behind
    `units_encoder.encode`, in place on its result, so the synthesiser - or every model's row gather - sees the blended units.
    `envelope`: None, or the envelope mix of the rows (rate_of_slot (S,) fp64 device, hop_in, hop_out, m, slot_of_row (rows,)
    int32 or None: row b is slot b): right behind the gate, `Context.envelope_rms` of the window at the device rate (hop_in),
    `Context.envelope_rms` of the gated signal at the model's rate (hop_out) and one `Context.envelope_mix_`, in place on the
    signal (RVC's `change_rms`; include/ddsp_amd.h states the rule).  A row whose rate is 1 keeps its bits.  Not with model=None.
    -> (signal (rows, Fr * block_size), f0 (rows, Fr, 1) after the shift, units (rows, Fr, C), volume (rows, Fr)), rows = 1 or S."""
    if push is None:
        ctx.stream_push_(window, block_in)
    else:
        push(ctx, window, block_in)
    audio = window if window.dim() == 2 else window[None]
    volume = ctx.volume_extract(audio, hop_size)
    f0 = f0_extractor.extract(window, uv_interp=True, silence_front=silence_front, dither=f0_dither, seed_dev=seed_dev)
    f0 = f0.reshape(-1, f0.shape[-1])[:, :, None]
    if isinstance(pitch, torch.Tensor):
        f0 = f0 * (pitch[:, :, None] if pitch.dim() == 2 else pitch[:, None, None])    # a factor per frame, or one per row
    elif pitch != 1:
        f0 = f0 * pitch
    if tune is not None:
        f0 = ctx.f0_tune_(f0.contiguous(), tune[0], tune[1], owner=tune[2])
    units = units_encoder.encode(audio, samplerate, hop_size)
    if retrieve is not None:
        bank, index_of_slot, ratio_of_slot, k, slot_of_row = retrieve
        units = ctx.units_retrieve_(units.contiguous(), bank, index_of_slot, ratio_of_slot, k=k, owner=slot_of_row)
    if model is None:
        if envelope is not None:
            raise ValueError("block_chain: envelope= needs the model (the signal is rendered here)")
        return None, f0, units, volume
    kw = {} if noise is None else {"noise": noise}
    sig = (model.forward_formant if "formant" in speaker else model)(units, f0, volume, **speaker, **kw)[0]
    ctx.volume_gate_(sig, volume, threshold_db, block_size)          # (`block_size`: the model's, as a host int - no read-back)
    if envelope is not None:
        rate_of_slot, hop_in, hop_out, m, slot_of_row = envelope
        ctx.envelope_mix_(sig, ctx.envelope_rms(audio, hop_in, m), rate_of_slot, ctx.envelope_rms(sig, hop_out, m), hop_out, hop_in,
                          int(audio.shape[1]), owner=slot_of_row)
    return sig, f0, units, volume


class GraphedBlock(_Captured):
    """`block_chain` for one fixed (window length, device rate, hop) as one linear HIP graph, over one window (n_in,) or S
    windows (S, n_in).  `window` is the caller's tensor: the graph shifts it in place at its fixed address, and the capture
    leaves its contents as it found them.  With `mix_rows=(mix_ids, mix_w)` these tables and a device `pitch` (S,) are the
    caller's too (`realtime.StreamBank`'s state): the graph reads them at their fixed addresses, so a write to a row between two
    replays is all a speaker, mix or pitch change takes.  Without it the speaker is the static input `spk_id` and the captured
    `spk_mix_dict`, and `pitch` a host factor.  `push`: `block_chain`'s; what it changes besides `window` it must leave alone
    while the capture runs (the bank's row table is all padding then), or name in `keep`: tensors of the caller's that the
    capture's runs change in place and that are put back as they were found, like `window` (a gliding bank's clocks).  With
    w (S, Fr, K) in `mix_rows` the mix is one per FRAME, and `push` fills it (`ddsp_bank_glide`).  `model=None`: the features alone (`block_chain`), `sig` is None and there is no `noise`.  Static inputs: `block_in`, `noise`, `seed`; static outputs (valid until the
    next replay): `sig`, `f0`, `units`, `volume`.  `tune`, `retrieve`, `envelope`: `block_chain`'s, the caller's device tensors, read at replay."""

    def __init__(self, model, units_encoder, f0_extractor, window, block, samplerate, hop_size, silence_front, pitch,
                 threshold_db, spk_mix_dict=None, mix_rows=None, f0_dither=True, warmup=3, push=None, keep=(), formant=None,
                 envelope=None, tune=None, retrieve=None):
        if mix_rows is not None and spk_mix_dict is not None:
            raise ValueError("GraphedBlock: mix_rows and spk_mix_dict are mutually exclusive")
        if mix_rows is not None and mix_rows[1].dim() == 3:          # a mix per FRAME: w (S, Fr, K), filled by `push`
            hipddsp.check_mix_frames(mix_rows[0], mix_rows[1], window.shape[0], int(window.shape[-1] // hop_size) + 1)
        dev = window.device if model is None else next(model.parameters()).device
        state = [window, *(mix_rows or ())] + ([pitch] if isinstance(pitch, torch.Tensor) else [])
        if dev.type != "cuda" or any(t.device != dev for t in state):
            raise RuntimeError("GraphedBlock needs the model and the caller's tensors on one HIP device (no CPU fallback)")
        self.model = None if model is None else model.eval()
        self.device = dev
        self.units_encoder, self.f0_extractor, self.window, self.pitch = units_encoder, f0_extractor, window, pitch
        self.args = (samplerate, hop_size, silence_front, float(threshold_db))
        self.f0_dither, self.push, self.tune, self.retrieve, self.envelope = bool(f0_dither), push, tune, retrieve, envelope
        rows = window.shape[:-1]                                     # () or (S,)
        frames = int(window.shape[-1] // hop_size) + 1
        self.block_size = None if model is None else int(model.block_size)
        self.block_in = torch.zeros(*rows, int(block), device=dev)
        self.spk_id = torch.ones(1, 1, dtype=torch.int64, device=dev) if mix_rows is None else None
        if mix_rows is None:
            self.speaker = {"spk_id": self.spk_id, "spk_mix_dict": None if spk_mix_dict is None else dict(spk_mix_dict)}
        else:
            self.speaker = {"spk_id": None, "spk_mix_rows": tuple(mix_rows)}
        if formant is not None:                                      # the caller's device factors (`forward_formant`), read at replay
            self.speaker["formant"] = formant
        self.noise = None if model is None else torch.rand(*(rows or (1,)), frames * self.block_size, device=dev)
        self.seed = torch.zeros(1, dtype=torch.int64, device=dev)
        self.sig, self.f0, self.units, self.volume = self._capture(dev, warmup, keep=[window, *keep])
        self.seed.random_(0, 2 ** 62)

    def _run(self):
        samplerate, hop_size, silence_front, threshold_db = self.args
        return block_chain(self.ctx, self.model, self.units_encoder, self.f0_extractor, self.window, self.block_in, samplerate,
                           hop_size, silence_front, self.pitch, threshold_db, self.block_size, self.speaker, self.noise,
                           self.f0_dither, self.seed, self.push, envelope=self.envelope, tune=self.tune, retrieve=self.retrieve)

    @torch.no_grad()
    def __call__(self, block_in, spk_id=None, noise=None):
        """block_in (block,) or (S, block) -> (sig, f0, units, volume) of the window(s) after they took it (static tensors).
        `spk_id` (1, 1): the solo form's speaker; the row form reads the caller's tables."""
        self.block_in.copy_(block_in.reshape(self.block_in.shape))
        if self.spk_id is not None:
            self.spk_id.copy_(spk_id.reshape(self.spk_id.shape))
        if self.noise is not None:
            _refill(self.noise, noise)
        self.graph.replay()
        return self.sig, self.f0, self.units, self.volume


def bank_enhancer_chain(ctx, enhancer, plan, sig, f0, request, rand_ini, model_sr, block_size, samplerate, n_end_by_key, tail_idx):
    """Steps 6-7 of the `StreamRenderer` chain over S rows, nothing read back: `enhancer.enhance_keyed` on the gated signal
    `sig` (S, Fr * block_size) and the shifted `f0` (S, Fr, 1) with the per-row key requests `request` (S,) int32 and the bank's
    `plan` (`enhancer.KeyedPlan`); `ddsp_resample` from the enhancer's rate to `samplerate` on the device lengths; then
    every row's last `tail_idx.numel()` samples counted from the row's OWN end (`gui.py:405-406` slices from the end), the
    end being `n_end_by_key[key]`.  -> (tail (S, n_tail), key (S,) int32)."""
    out, sr_e, n_out, key = enhancer.enhance_keyed(sig, model_sr, f0, block_size, adaptive_key=request,
                                                   silence_front=plan.silence_front, max_key=plan.max_key, rand_ini=rand_ini, plan=plan)
    if int(sr_e) != int(samplerate):
        out = ctx.resample(out, int(sr_e), int(samplerate), 128, n_dev=n_out)
    n_end = n_end_by_key.index_select(0, key.long())
    idx = (n_end.long() - tail_idx.numel())[:, None] + tail_idx[None, :]
    return out.gather(1, idx), key


class GraphedBankEnhancer(_Captured):
    """`bank_enhancer_chain` for S rows of one geometry as one linear HIP graph.  `request` is the caller's tensor (the bank's
    table of key requests, read at its fixed address).  Static inputs: `sig`, `f0`, `rand_ini` (S, 9), refilled before every
    replay; static outputs (valid until the next replay): `tail`, `key`.  The plan's tap tables and device tables are built by
    the warm-up runs, before the capture."""

    def __init__(self, enhancer, plan, S, request, model_sr, block_size, samplerate, n_end_by_key, tail_idx, warmup=3):
        self.device = dev = request.device
        if dev.type != "cuda":
            raise RuntimeError("GraphedBankEnhancer needs the bank's state on a HIP device (no CPU fallback)")
        self.enhancer, self.plan, self.request = enhancer, plan, request
        self.args = (int(model_sr), int(block_size), samplerate, n_end_by_key, tail_idx)
        self.sig = torch.zeros(S, plan.T, device=dev)
        self.f0 = torch.full((S, plan.Fr, 1), 220.0, device=dev)
        self.rand_ini = torch.rand(S, 9, device=dev)
        self.tail, self.key = self._capture(dev, warmup)

    def _run(self):
        model_sr, block_size, samplerate, n_end_by_key, tail_idx = self.args
        return bank_enhancer_chain(self.ctx, self.enhancer, self.plan, self.sig, self.f0, self.request, self.rand_ini, model_sr,
                                   block_size, samplerate, n_end_by_key, tail_idx)

    @torch.no_grad()
    def __call__(self, sig, f0, rand_ini=None):
        """sig (S, Fr * block_size), f0 (S, Fr, 1) -> (tail, key) (static tensors)."""
        self.sig.copy_(sig.reshape(self.sig.shape))
        self.f0.copy_(f0.reshape(self.f0.shape))
        _refill(self.rand_ini, None if rand_ini is None else rand_ini.reshape(-1, 9).expand_as(self.rand_ini))
        self.graph.replay()
        return self.tail, self.key
