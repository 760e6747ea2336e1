"""`Unit2Control` with the reference's constructor, state-dict keys and forward contract
(reference `ddsp/unit2control.py:23-101`, `ddsp/pcmer.py`), executed by libddsp_amd.

The torch modules below are PARAMETER CONTAINERS only (their names reproduce the reference's
state-dict layout so upstream checkpoints load with `load_state_dict`); none of them has a forward of
its own.  `Unit2Control.forward` hands raw device pointers to `ddsp_unit2ctrl_fwd`.
"""
import math

import torch
import torch.nn as nn

import hipddsp

NDIM = 256
N_LAYERS = 3
N_HEADS = 8
HEAD_DIM = 64
N_FEATURES = int(HEAD_DIM * math.log(HEAD_DIM))  # 266 random features (reference ddsp/pcmer.py:196)
DW_KERNEL = 31


def is_frame_mix(spk_mix_rows):
    """True for the per-FRAME form of `spk_mix_rows`: a pair (ids (B, K), w (B, Fr, K)) - the weights have a frame axis."""
    return isinstance(spk_mix_rows, (tuple, list)) and len(spk_mix_rows) == 2 and isinstance(spk_mix_rows[1], torch.Tensor) \
        and spk_mix_rows[1].dim() == 3


def mix_frames_of_dict(spk_mix_dict, B, Fr, device, n_spk):
    """The reference's `spk_mix_dict` with TENSOR values -> the per-frame tables (ids (B, K) int32, w (B, Fr, K) fp32) on
    `device`, or None for a dict whose values are all numbers (the one host mix of the batch, handled as ever).  A value is a
    tensor of shape (B, Fr, 1), (1, Fr, 1), (B, Fr), (1, Fr) or (Fr,) - what broadcasts against the reference's (B, Fr, 256)
    activations, with (Fr,) read as one weight per frame - or a number, constant over the call.  Slots are in dict order, as
    the reference's loop adds them.  ValueError for another shape, no or more than `hipddsp.MAX_MIX` ids, an id outside
    [1, n_spk]."""
    if not isinstance(spk_mix_dict, dict) or not any(isinstance(v, torch.Tensor) and v.dim() >= 1 for v in spk_mix_dict.values()):
        return None
    if not 1 <= len(spk_mix_dict) <= hipddsp.MAX_MIX:
        raise ValueError(f"spk_mix_dict: a speaker mix holds 1 to {hipddsp.MAX_MIX} ids, got {len(spk_mix_dict)}")
    cols = []
    for i, v in spk_mix_dict.items():
        if not 1 <= int(i) <= int(n_spk):
            raise ValueError(f"spk_mix_dict: speaker id {i} is outside [1, {int(n_spk)}]")
        if not (isinstance(v, torch.Tensor) and v.dim() >= 1):
            cols.append(torch.full((B, Fr), float(v), dtype=torch.float32, device=device))
            continue
        shape = tuple(v.shape)
        if shape not in ((B, Fr, 1), (1, Fr, 1), (B, Fr), (1, Fr), (Fr,)):
            raise ValueError(f"spk_mix_dict: the weights of speaker {i} have shape {shape}; a per-frame weight is (B, Fr, 1), "
                             f"(1, Fr, 1) or (Fr,) with B = {B}, Fr = {Fr}")
        cols.append(v.to(device=device, dtype=torch.float32).reshape(-1, Fr).expand(B, Fr))
    ids = torch.tensor([[int(i) for i in spk_mix_dict]] * B, dtype=torch.int32).to(device)
    return ids, torch.stack(cols, dim=2).contiguous()


class _Slot(nn.Module):
    """Placeholder keeping the index of a parameter-free layer inside an nn.Sequential."""


def _uniform_(t, bound):
    with torch.no_grad():
        return t.uniform_(-bound, bound)


class _Affine(nn.Module):
    """weight/bias pair initialised like torch's Linear / Conv1d (kaiming-uniform, a=sqrt(5))."""

    def __init__(self, w_shape, fan_in, ones=False):
        super().__init__()
        if ones:  # normalisation layers
            self.weight = nn.Parameter(torch.ones(w_shape))
            self.bias = nn.Parameter(torch.zeros(w_shape))
        else:
            bound = 1.0 / math.sqrt(fan_in)
            self.weight = nn.Parameter(_uniform_(torch.empty(w_shape), bound))
            self.bias = nn.Parameter(_uniform_(torch.empty(w_shape[0]), bound))


class _WeightNormHead(nn.Module):
    """Keys bias / weight_g / weight_v of the reference's `weight_norm(nn.Linear(...))` (:61)."""

    def __init__(self, n_in, n_out):
        super().__init__()
        bound = 1.0 / math.sqrt(n_in)
        v = _uniform_(torch.empty(n_out, n_in), bound)
        self.bias = nn.Parameter(_uniform_(torch.empty(n_out), bound))
        self.weight_g = nn.Parameter(v.norm(dim=1, keepdim=True).clone())
        self.weight_v = nn.Parameter(v)


def _orthogonal_gaussian_features(n_rows, n_cols):
    """Performer projection: stacked orthogonal blocks with chi-distributed row norms (the construction
    the reference uses for its fixed `projection_matrix` buffer, `ddsp/pcmer.py:80-120`)."""
    blocks = []
    remaining = n_rows
    while remaining > 0:
        q, _ = torch.linalg.qr(torch.randn(n_cols, n_cols), mode="reduced")
        take = min(remaining, n_cols)
        blocks.append(q.t()[:take])
        remaining -= take
    mat = torch.cat(blocks, dim=0)
    norms = torch.randn(n_rows, n_cols).norm(dim=1)
    return norms[:, None] * mat


class _FastAttention(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("projection_matrix", _orthogonal_gaussian_features(N_FEATURES, HEAD_DIM))


class _SelfAttention(nn.Module):
    def __init__(self, dim):
        super().__init__()
        inner = N_HEADS * HEAD_DIM
        self.fast_attention = _FastAttention()
        self.to_q = _Affine((inner, dim), dim)
        self.to_k = _Affine((inner, dim), dim)
        self.to_v = _Affine((inner, dim), dim)
        self.to_out = _Affine((dim, inner), inner)


class _ConvModule(nn.Module):
    def __init__(self, dim):
        super().__init__()
        inner = dim * 2
        self.net = nn.Sequential(
            _Affine((dim,), dim, ones=True),                 # 0 LayerNorm
            _Slot(),                                         # 1 transpose
            _Affine((inner * 2, dim, 1), dim),               # 2 pointwise conv
            _Slot(),                                         # 3 GLU
            _Affine((inner, 1, DW_KERNEL), DW_KERNEL),       # 4 depthwise conv
            _Slot(),                                         # 5 SiLU
            _Affine((dim, inner, 1), inner),                 # 6 pointwise conv
            _Slot(), _Slot(),                                # 7 transpose, 8 dropout(p=0)
        )


class _EncoderLayer(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm = _Affine((dim,), dim, ones=True)
        self.attn = _SelfAttention(dim)
        self.local_mixer = _ConvModule(dim)


class _PCmer(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.net = nn.Sequential(*[_EncoderLayer(dim) for _ in range(N_LAYERS)])


def split_to_dict(tensor, tensor_splits):
    """Views into the fused control matrix, in dict order (reference `ddsp/unit2control.py:10-20`)."""
    out = {}
    lo = 0
    for name, width in tensor_splits.items():
        out[name] = tensor[..., lo:lo + width]
        lo += width
    return out


class Unit2Control(nn.Module):
    def __init__(self, ndim_feat_i, n_spk, output_splits, c=False):
        super().__init__()
        # c = True: causal convolutions (taps at frames t-k+1 .. t) and causal linear attention, forward and backward.  The two
        # third-party primitives behind it (extorch.Conv1dEx(causal=True), fast_transformers.CausalDotProduct) are not in
        # the image: they are restated from their definitions, parity at that boundary is unpinned.
        self.causal = bool(c)
        self.n_unit = int(ndim_feat_i)
        self.n_spk = int(n_spk)
        self.output_splits = dict(output_splits)
        self.n_out = sum(self.output_splits.values())
        self.unit_prenet = nn.Sequential(
            _Slot(),
            _Affine((NDIM, self.n_unit, 3), self.n_unit * 3),
            _Affine((NDIM,), NDIM, ones=True),               # GroupNorm(4, 256)
            _Slot(),
            _Affine((NDIM, NDIM, 3), NDIM * 3),
            _Slot(),
        )
        self.f0_embed = _Affine((NDIM, 1), 1)
        self.phase_embed = _Affine((NDIM, 1), 1)
        self.volume_embed = _Affine((NDIM, 1), 1)
        self.spk_embed = nn.Module()
        self.spk_embed.weight = nn.Parameter(torch.randn(self.n_spk, NDIM))
        self.dec_post = nn.Sequential(_PCmer(NDIM), _Affine((NDIM,), NDIM, ones=True),
                                      _WeightNormHead(NDIM, self.n_out))
        self._table = hipddsp.WeightTable(hipddsp.U2CWeights, Unit2Control._named_tensors, "Unit2Control", copy=True,
                                          grad_uncached=True, n_spk=self.n_spk, n_unit=self.n_unit, n_out=self.n_out,
                                          causal=int(self.causal))

    # ---- raw pointer table ---------------------------------------------------------------------
    def _named_tensors(self):
        """(struct field, tensor) pairs in the order of `ddsp_u2c_weights`."""
        pre = self.unit_prenet
        out = [("prenet_conv1_w", pre[1].weight), ("prenet_conv1_b", pre[1].bias), ("prenet_gn_w", pre[2].weight),
               ("prenet_gn_b", pre[2].bias), ("prenet_conv2_w", pre[4].weight), ("prenet_conv2_b", pre[4].bias),
               ("f0_w", self.f0_embed.weight), ("f0_b", self.f0_embed.bias), ("phase_w", self.phase_embed.weight),
               ("phase_b", self.phase_embed.bias), ("volume_w", self.volume_embed.weight),
               ("volume_b", self.volume_embed.bias), ("spk_table", self.spk_embed.weight)]
        for i, layer in enumerate(self.dec_post[0].net):
            a, cm = layer.attn, layer.local_mixer.net
            vals = dict(norm_w=layer.norm.weight, norm_b=layer.norm.bias,
                        q_w=a.to_q.weight, q_b=a.to_q.bias, k_w=a.to_k.weight, k_b=a.to_k.bias,
                        v_w=a.to_v.weight, v_b=a.to_v.bias, proj=a.fast_attention.projection_matrix,
                        out_w=a.to_out.weight, out_b=a.to_out.bias,
                        cm_ln_w=cm[0].weight, cm_ln_b=cm[0].bias, cm_pw1_w=cm[2].weight, cm_pw1_b=cm[2].bias,
                        cm_dw_w=cm[4].weight, cm_dw_b=cm[4].bias, cm_pw2_w=cm[6].weight, cm_pw2_b=cm[6].bias)
            out += [(f"l{i}_{k}", v) for k, v in vals.items()]
        head = self.dec_post[2]
        out += [("final_ln_w", self.dec_post[1].weight), ("final_ln_b", self.dec_post[1].bias),
                ("head_g", head.weight_g), ("head_v", head.weight_v), ("head_b", head.bias)]
        return out

    def backward_flat(self, units, f0, phase, volume, spk_id, spk_mix_dict, d_ctrl, ctx=None, kept=None, n_frames=None,
                      n_dev=None):
        """Gradients of every parameter for an upstream d_ctrl (B,Fr,n_out): {parameter tensor: gradient tensor}.
        `ctx`: the context of the forward call (autograd runs backward on its own thread; reusing the forward's
        context keeps one scratch arena and one profiler per model call).  `kept`: the activation region of a
        `forward_flat_keep` call on the same inputs and weights - without it the forward is re-run inside the call.
        `n_frames` (as `forward_flat` takes it): a ragged batch - every gradient is the sum over rows of the gradient that row
        gives alone at its own length, whatever the padding of the inputs and of d_ctrl holds.  `n_dev` instead: the counts
        on the device, with the inputs already in held form (`hold_ragged`) and d_ctrl 0 on every row's padding - what
        the synthesisers' autograd node passes."""
        ctx = ctx or hipddsp.context_for(units.device)
        if n_frames is not None:
            vals = self.check_ragged(n_frames, units.shape[0], units.shape[1])
            n_dev, units, f0, phase, volume = self.hold_ragged(ctx, vals, units, f0, phase, volume)
            d_ctrl = ctx.ragged_frames(d_ctrl, n_dev, hold=False)
        w, keep = self._weights_struct()
        g = hipddsp.U2CWeights()
        grads = {}
        # `training.GradBucket.zero()` arms `_grads_in_place`: the library then writes every gradient straight into the
        # parameter's `.grad` (a view of the bucket's freshly zeroed flat buffer) and autograd gets nothing to accumulate - no
        # per-parameter add launches (0.18 ms of a B = 32 step).  The library WRITES (`=`), so the token is consumed here: a
        # second backward pass before the next `zero()` returns its gradients to autograd, which accumulates them.
        in_place = getattr(self, "_grads_in_place", False)
        self._grads_in_place = False
        for name, t in self._named_tensors():
            if name.endswith("_proj"):
                continue
            if in_place and t.grad is not None and t.grad.is_contiguous() and t.grad.dtype == torch.float32:
                setattr(g, name, t.grad.data_ptr())
                continue
            gt = torch.empty_like(t, dtype=torch.float32, memory_format=torch.contiguous_format)
            grads[t] = gt
            setattr(g, name, gt.data_ptr())
        g.n_spk, g.n_unit, g.n_out = self.n_spk, self.n_unit, self.n_out
        if kept is not None:
            ctx.unit2ctrl_bwd_kept(w, g, units, f0, phase, volume, spk_id, spk_mix_dict, kept, d_ctrl, n_frames=n_dev)
        else:
            ctx.unit2ctrl_bwd(w, g, units, f0, phase, volume, spk_id, spk_mix_dict, self.n_out, d_ctrl, n_frames=n_dev)
        return grads

    def rebind(self):
        """Forget the weight struct and have the library re-prepare the weights: after a submodule of this network was replaced,
        or after a write `_version` does not count (`hipddsp.WeightTable`)."""
        self._table.invalidate()

    def _weights_struct(self):
        return self._table.struct(self)

    def forward_flat(self, units, f0, phase, volume, spk_id, spk_mix_dict=None, n_frames=None, spk_mix_rows=None):
        """(B, Fr, n_out) fused control matrix (the split views are taken by `forward`).
        `spk_mix_rows` (ids (B, K) int32, w (B, K) fp32, device tensors): a speaker mix per row in place of `spk_id` /
        `spk_mix_dict` (`hipddsp.check_mix_rows`; inference only, the callers check that).  With w (B, Fr, K) the pair is a mix
        per FRAME (`hipddsp.check_mix_frames`): frame i of row b adds sum_k w[b, i, k] * spk_embed[ids[b, k] - 1].  A
        `spk_mix_dict` with tensor values ((B, Fr, 1), (1, Fr, 1) or (Fr,), the reference's broadcast) is turned into that form
        (`mix_frames_of_dict`); both refuse a network that wants gradients (NotImplementedError).
        `n_frames` (a sequence of B ints or a CPU integer tensor (B,), 1 <= n_frames[b] <= Fr): a ragged batch - the first
        n_frames[b] rows of ctrl[b] are what the network gives for that row alone at its own length, whatever the padding of
        the inputs holds; the rows after them carry no meaning.  Inference only: this call records nothing for autograd
        (NotImplementedError with grad mode on and a parameter that wants a gradient); the training pair of a ragged batch is
        `forward_ragged_keep` / `backward_flat(n_frames= | n_dev=)`."""
        spk_mix_dict, spk_mix_rows = self.frame_mix(spk_mix_dict, spk_mix_rows, units.shape[0], units.shape[1], units.device)
        if n_frames is not None:
            vals = self.check_ragged(n_frames, units.shape[0], units.shape[1])
            if self.wants_grad():
                raise NotImplementedError("forward_flat(n_frames=) is inference only: it records nothing for autograd; call it "
                                          "under torch.no_grad() (training: forward_ragged_keep / backward_flat)")
            ctx = hipddsp.context_for(units.device)
            n_dev, units, f0, phase, volume = self.hold_ragged(ctx, vals, units, f0, phase, volume)
            return self.forward_ragged(ctx, units, f0, phase, volume, spk_id, spk_mix_dict, n_dev, hold=False,
                                       spk_mix_rows=self.hold_frame_mix(ctx, spk_mix_rows, n_dev))
        ctx = hipddsp.context_for(units.device)
        return self._control(ctx, units, f0, phase, volume, spk_id, spk_mix_dict, None, spk_mix_rows)

    def frame_mix(self, spk_mix_dict, spk_mix_rows, B, Fr, device):
        """Head of a call that may carry a mix per frame, before anything is launched -> (spk_mix_dict, spk_mix_rows) as the
        rest of the call takes them: a `spk_mix_dict` with tensor values becomes the pair (ids, w (B, Fr, K)) and the dict
        None; a per-frame pair is checked (`hipddsp.check_mix_frames`, ValueError) and refused with a dict beside it or on a
        network that wants gradients (inference only, as the row mix); everything else passes through."""
        made = mix_frames_of_dict(spk_mix_dict, B, Fr, device, self.n_spk) if spk_mix_rows is None else None
        if made is not None:
            spk_mix_dict, spk_mix_rows = None, made
        if is_frame_mix(spk_mix_rows):
            if spk_mix_dict is not None:
                raise ValueError("a speaker mix per frame (device tables) and spk_mix_dict (one host mix for the batch) are "
                                 "mutually exclusive")
            hipddsp.check_mix_frames(spk_mix_rows[0], spk_mix_rows[1], B, Fr)
            if self.wants_grad():
                raise NotImplementedError("a speaker mix per frame is inference only: the training entries take spk_id or a "
                                          "spk_mix_dict of numbers; call the model under torch.no_grad()")
        return spk_mix_dict, spk_mix_rows

    @staticmethod
    def hold_frame_mix(ctx, spk_mix_rows, n_dev):
        """The weights of a per-frame mix 0 past every row's count, like the other frame-rate inputs of a ragged call
        (`hold_ragged`): what their padding holds never reaches arithmetic.  Another `spk_mix_rows` passes through."""
        if not is_frame_mix(spk_mix_rows):
            return spk_mix_rows
        return spk_mix_rows[0], ctx.ragged_frames(spk_mix_rows[1], n_dev, hold=False)

    def _control(self, ctx, units, f0, phase, volume, spk_id, spk_mix_dict, n_dev, spk_mix_rows):
        """The one library call of an inference forward: the per-frame mix has a binding method of its own."""
        w, keep = self._weights_struct()
        if is_frame_mix(spk_mix_rows):
            return ctx.unit2ctrl_framemix(w, units, f0, phase, volume, spk_mix_rows[0], spk_mix_rows[1], self.n_out, n_frames=n_dev)
        return ctx.unit2ctrl(w, units, f0, phase, volume, spk_id, spk_mix_dict, self.n_out, n_frames=n_dev, mix_dev=spk_mix_rows)

    def wants_grad(self):
        """True when a call must be recorded for autograd (grad mode on and some parameter wants a gradient)."""
        return torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    def check_ragged(self, n_frames, B, Fr):
        """Head of a ragged call, host half, before anything is launched: `n_frames` as a checked list (ValueError).  (What a
        caller refuses under grad mode is its own business: the synthesisers an eval-mode model, `forward_flat` every call.)"""
        return hipddsp.check_n_frames(n_frames, B, Fr)

    def hold_ragged(self, ctx, vals, units, f0, phase, volume):
        """Head of a ragged call, device half: uploads the counts once and puts the frame-rate inputs into held form - units,
        volume and a given phase (None: the caller scans it from the held f0) 0, f0 its last frame over a row's padding
        (`csrc/ragged.hip`).  The padding is replaced by selection before anything reads it (the chunked causal attention,
        for one, multiplies a whole 16-frame tile before it masks: a NaN there would not stay in its own frame).
        -> (n_dev, units, f0 (B,Fr), phase (B,Fr) | None, volume (B,Fr))."""
        B, Fr = units.shape[0], units.shape[1]
        n_dev = ctx.ragged_counts(vals)
        frames = lambda x, hold: ctx.ragged_frames(x.reshape(B, Fr), n_dev, hold=hold)
        return (n_dev, ctx.ragged_frames(units, n_dev, hold=False), frames(f0, True),
                None if phase is None else frames(phase, False), frames(volume, False))

    def forward_ragged(self, ctx, units, f0, phase, volume, spk_id, spk_mix_dict, n_dev, hold=True, spk_mix_rows=None):
        """The control matrix of a ragged batch whose counts are on the device (`Context.ragged_counts`) and whose units are 0
        past every row's count.  hold: every row's last control frame is repeated over its padding - the form in which the
        DSP kernels take a ragged batch (`csrc/ragged.hip`).  The weights of a per-frame `spk_mix_rows` are finite past every
        row's count (`hold_frame_mix`)."""
        ctrl = self._control(ctx, units, f0, phase, volume, spk_id, spk_mix_dict, n_dev, spk_mix_rows)
        return ctx.ragged_frames(ctrl, n_dev, hold=True, out=ctrl) if hold else ctrl

    def forward_flat_keep(self, units, f0, phase, volume, spk_id, spk_mix_dict=None, ctx=None):
        """Training forward: (control matrix, kept activations) - PyTorch keeps a module's activations for `backward`
        (reference `solver.py:111-113`); here the library leaves them in one device region that `backward_flat(kept=...)`
        starts from, so the network runs once per step."""
        ctx = ctx or hipddsp.context_for(units.device)
        w, keep = self._weights_struct()
        return ctx.unit2ctrl_keep(w, units, f0, phase, volume, spk_id, spk_mix_dict, self.n_out)

    def forward_ragged_keep(self, ctx, units, f0, phase, volume, spk_id, spk_mix_dict, n_dev, hold=True):
        """`forward_flat_keep` of a ragged batch in the form `forward_ragged` takes (counts on the device, inputs from
        `hold_ragged`): (control matrix, kept activations) for `backward_flat(kept=..., n_dev=...)` on the same inputs.  hold:
        as there - its adjoint, `Context.ragged_frames_adjoint_`, is then the caller's to apply to d_ctrl."""
        w, keep = self._weights_struct()
        ctrl, kept = ctx.unit2ctrl_keep(w, units, f0, phase, volume, spk_id, spk_mix_dict, self.n_out, n_frames=n_dev)
        return (ctx.ragged_frames(ctrl, n_dev, hold=True, out=ctrl) if hold else ctrl), kept

    def forward(self, units, f0, phase, volume, spk_id, spk_mix_dict=None):
        """Same contract as the reference `Unit2Control.forward` (`ddsp/unit2control.py:68-101`):
        units (B,Fr,n_unit), f0 (B,Fr,1), phase (B,Fr), volume (B,Fr), spk_id (B,1)|(1,1) int64 1-based,
        spk_mix_dict {id: weight} or None -> dict of (B,Fr,width) views."""
        return split_to_dict(self.forward_flat(units, f0, phase, volume, spk_id, spk_mix_dict), self.output_splits)
