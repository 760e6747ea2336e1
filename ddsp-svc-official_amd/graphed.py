"""HIP-graph replay of a synthesiser's inference forward for one fixed (batch, frames) shape.

The real-time caller (`gui.py:360-430`: one 0.2 s block at a time, B = 1, 87 frames) is launch-bound: ~50 kernels of
a few microseconds each, paced by Python + ctypes + hipLaunch on the host.  `GraphedSynth` captures the whole
`model(...)` call once (`torch.cuda.graph`: stream capture also records the kernels libddsp_amd launches on that
stream) and replays it with one host call per block.

What makes the capture safe:
  * the model's library calls go through a `hipddsp.Context` of their own (`hipddsp.use_context`): the captured kernels
    point into THAT context's scratch arena, tables and zero page, which are sized by eager warm-up runs before the
    capture and frozen afterwards (`Context.freeze`) - no later eager call can regrow or reuse them;
  * the noise excitation comes from a static device tensor that is refilled before every replay (the eager path draws
    a host seed per call, which a graph would freeze);
  * inputs are copied into static tensors, outputs are static tensors valid until the next replay.
Weights are read by the captured kernels at replay time (the weight-preparation kernel is part of the graph), so
in-place weight updates are honoured.  `spk_mix_dict` ({speaker id: weight}) is captured with the graph: its ids and
weights become kernel arguments, so a capture is valid for that mix only (a new mix needs a new `GraphedSynth`;
`realtime.StreamRenderer.set_speaker` does that), while `spk_id` stays a static input.  `initial_phase` is a host-side
argument and not supported here.  Forward only.

`GraphedBlock` captures the real-time block from the raw audio on (`block_chain`: window push, volume, f0 extractor, pitch
shift, units encoder, synthesiser, volume gate) under the same rules, on one stream (a linear graph).  Three networks then
share the captured context; each has a prepared-weight slot of its own in it.  The control network's weights are prepared
inside the graph on every replay (in-place updates are honoured, as above); the two analysis networks (HuBERT-Soft, CREPE:
inference only) are prepared once by the warm-up runs and the captured kernels read those copies
(`ddsp_weight_slot_take(..., keep_in_capture)`), so a change of THEIR weights needs a new capture.  The CREPE dither seed lives
in a device word that the decode advances (`ddsp_crepe_decode_dseed`): a seed passed by value would be frozen by the capture.
"""
import torch

import hipddsp


class GraphedSynth:
    def __init__(self, model, B, Fr, warmup=3, spk_mix_dict=None):
        p = next(model.parameters())
        if not p.is_cuda:
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
        self.ctx = hipddsp.Context(dev)
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side), hipddsp.use_context(self.ctx), torch.no_grad():
            for _ in range(max(1, warmup)):          # first-use allocations (arena, tables) happen here, eagerly
                self._run()
        cur.wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with hipddsp.use_context(self.ctx), torch.no_grad(), torch.cuda.graph(self.graph):
            self.out = self._run()
        self.ctx.freeze()

    def _run(self):
        return self.model(self.units, self.f0, self.volume, self.spk_id, spk_mix_dict=self.spk_mix_dict, noise=self.noise)

    @torch.no_grad()
    def __call__(self, units, f0, volume, spk_id, noise=None):
        """Same positional inputs as `model.forward`; returns the model's result tuple (static tensors, overwritten by
        the next call).  `noise` (B, T) in [0, 1) replaces the fresh uniform draw (parity tests)."""
        if tuple(units.shape[:2]) != (self.B, self.Fr):
            raise ValueError(f"GraphedSynth captured for (B, Fr) = {(self.B, self.Fr)}, got {tuple(units.shape[:2])}")
        self.units.copy_(units)
        self.f0.copy_(f0.reshape(self.f0.shape))
        self.volume.copy_(volume.reshape(self.volume.shape))
        self.spk_id.copy_(spk_id.expand_as(self.spk_id) if spk_id.shape[0] == 1 else spk_id.reshape(self.spk_id.shape))
        if noise is None:
            self.noise.uniform_()
        else:
            self.noise.copy_(noise)
        self.graph.replay()
        return self.out


def block_chain(ctx, model, units_encoder, f0_extractor, window, block_in, samplerate, hop_size, silence_front, pitch_factor,
                threshold_db, block_size, spk_id, spk_mix_dict=None, noise=None, f0_dither=True, seed_dev=None):
    """One block of the reference's callback from the raw audio to the gated model output (gui.py:373-374 and
    `gui.SvcDDSP.infer`, gui.py:87-127), every step on the device, nothing read back:
    `window` (n_in,) takes `block_in` in place, then volume, f0 (uv_interp, silent front), the pitch shift, units, the
    synthesiser and the gate.  -> (signal (1, Fr * block_size), f0 (1, Fr, 1) after the shift, units (1, Fr, C), volume (1, Fr))."""
    ctx.stream_push_(window, block_in)
    volume = ctx.volume_extract(window[None], hop_size)
    f0 = f0_extractor.extract(window, uv_interp=True, silence_front=silence_front, dither=f0_dither, seed_dev=seed_dev)
    f0 = f0[None, :, None]
    if pitch_factor != 1:
        f0 = f0 * pitch_factor
    units = units_encoder.encode(window[None], samplerate, hop_size)
    kw = {} if noise is None else {"noise": noise}
    sig = model(units, f0, volume, spk_id, spk_mix_dict=spk_mix_dict, **kw)[0]
    ctx.volume_gate_(sig, volume, threshold_db, block_size)          # (`block_size`: the model's, as a host int - no read-back)
    return sig, f0, units, volume


class GraphedBlock:
    """`block_chain` for one fixed (window length, device rate, hop) as one HIP graph.  `window` is the caller's tensor: the
    graph shifts it in place at its fixed address, and the warm-up runs leave its contents as they found them (a re-capture
    in the middle of a stream keeps the stream).  Static inputs: `block_in`, `spk_id`, `noise`, `seed`; static outputs
    (valid until the next replay): `sig`, `f0`, `units`, `volume`."""

    def __init__(self, model, units_encoder, f0_extractor, window, block, samplerate, hop_size, silence_front, pitch_factor,
                 threshold_db, spk_mix_dict=None, f0_dither=True, warmup=3):
        p = next(model.parameters())
        if not p.is_cuda or window.device != p.device:
            raise RuntimeError("GraphedBlock needs the model and the window on one HIP device (no CPU fallback)")
        self.model = model.eval()
        self.device = dev = p.device
        self.units_encoder, self.f0_extractor, self.window = units_encoder, f0_extractor, window
        self.args = (samplerate, hop_size, silence_front, pitch_factor, float(threshold_db))
        self.spk_mix_dict = None if spk_mix_dict is None else dict(spk_mix_dict)
        self.f0_dither = bool(f0_dither)
        frames = int(window.numel() // hop_size) + 1
        self.block_size = int(model.block_size)
        self.block_in = torch.zeros(int(block), device=dev)
        self.spk_id = torch.ones(1, 1, dtype=torch.int64, device=dev)
        self.noise = torch.rand(1, frames * self.block_size, device=dev)
        self.seed = torch.zeros(1, dtype=torch.int64, device=dev)
        self.ctx = hipddsp.Context(dev)
        kept = window.clone()
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side), hipddsp.use_context(self.ctx), torch.no_grad():
            for _ in range(max(1, warmup)):   # arena, tap tables and the analysis networks' prepared weights: here, eagerly
                self._run()
        cur.wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with hipddsp.use_context(self.ctx), torch.no_grad(), torch.cuda.graph(self.graph):
            self.sig, self.f0, self.units, self.volume = self._run()
        self.ctx.freeze()
        window.copy_(kept)
        self.seed.random_(0, 2 ** 62)

    def _run(self):
        samplerate, hop_size, silence_front, pitch_factor, threshold_db = self.args
        return block_chain(self.ctx, self.model, self.units_encoder, self.f0_extractor, self.window, self.block_in, samplerate,
                           hop_size, silence_front, pitch_factor, threshold_db, self.block_size, self.spk_id, self.spk_mix_dict,
                           self.noise, self.f0_dither, self.seed)

    @torch.no_grad()
    def __call__(self, block_in, spk_id, noise=None):
        """block_in (block,) -> (sig, f0, units, volume) of the window after it took the block (static tensors)."""
        self.block_in.copy_(block_in.reshape(self.block_in.shape))
        self.spk_id.copy_(spk_id.reshape(self.spk_id.shape))
        if noise is None:
            self.noise.uniform_()
        else:
            self.noise.copy_(noise)
        self.graph.replay()
        return self.sig, self.f0, self.units, self.volume
