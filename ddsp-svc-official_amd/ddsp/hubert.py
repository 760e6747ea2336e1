"""HuBERT units encoders executed by libddsp_amd: HuBERT-Soft (the reference's `encoder/hubert/model.py` `HubertSoft`) and
the HuBERT-base form of fairseq (`HubertBase`: ContentVec and HuBERT-base checkpoints, reference `ddsp/vocoder.py:231-332`).

`HubertSoft` has exactly the reference's state-dict keys and shapes (166, including `masked_spec_embed` and
`label_embedding.weight`, which `units` does not read), so the released checkpoint loads with `strict=True`.
`units(wav (B,1,T)) -> (B, Fr, 256)` runs on the device only (a CPU tensor raises RuntimeError); `encode(wav, layer)` gives
the conv stack's output (layer=-1) or the hidden state after `layer` transformer layers.  Inference only: nothing here
records gradients (the reference runs the encoder under `torch.inference_mode`).

`HubertBase` has fairseq's `HubertModel` keys and shapes for the base architecture, so a fairseq state dict loads with
`strict=True` (`load_fairseq_state`, `read_fairseq_checkpoint`).  It is the same network with three differences: the audio
is not padded, `units(wav, layer=9, project=True)` stops after `layer` transformer layers and returns that hidden state (768
wide) or its `final_proj` (256 wide), and the attention's q / k / v projections are separate tensors, which the library packs
into its QKV operand when it prepares the weights.

The library keeps its prepared copies of the weights (repacked convolutions, the folded weight norm, the packed QKV
operands) while the parameters' values stand, as `hipddsp.WeightTable` describes: a write that torch does not count (into
`p.data`) needs `rebind()`.
"""
import pickle

import torch
from torch import nn

import hipddsp

SAMPLE_RATE = 16000
HOP_SIZE = 320


def n_frames(T):
    """Encoder frames of T samples at 16 kHz (`ddsp_hubert_frames`); ValueError when the audio is too short for the conv stack."""
    n = hipddsp.hubert_frames(int(T))
    if n <= 0:
        raise ValueError(f"HubertSoft: {int(T)} samples are too short for the conv stack")
    return n


class RaggedCounts:
    """Checked per-row sample counts of a ragged batch together with their (B,) int32 device tensor (`HubertSoft.counts`):
    pass it as `n_samples=` to skip the host check and the upload, e.g. inside a HIP graph capture, where nothing may be
    uploaded.  The caller keeps it alive as long as a captured graph reads it."""

    def __init__(self, values, T, dev_tensor):
        self.values, self.T, self.dev = list(values), int(T), dev_tensor


class _WeightNormConv(nn.Module):
    """`positional_embedding.conv` after `weight_norm(dim=2)`: its keys are `bias`, `weight_g`, `weight_v`."""

    def __init__(self):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(768))
        self.weight_g = nn.Parameter(torch.ones(1, 1, 128))
        self.weight_v = nn.Parameter(torch.zeros(768, 48, 128))


class _Linear(nn.Module):
    def __init__(self, n_in, n_out):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(n_out, n_in))
        self.bias = nn.Parameter(torch.zeros(n_out))


class _Norm(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(n))
        self.bias = nn.Parameter(torch.zeros(n))


class _Conv(nn.Module):
    def __init__(self, c_in, c_out, k):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(c_out, c_in, k))


class _Attention(nn.Module):
    def __init__(self):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.zeros(2304, 768))
        self.in_proj_bias = nn.Parameter(torch.zeros(2304))
        self.out_proj = _Linear(768, 768)


class _Layer(nn.Module):
    """`nn.TransformerEncoderLayer(768, 12, 3072, activation="gelu", batch_first=True)`, post-norm."""

    def __init__(self):
        super().__init__()
        self.self_attn = _Attention()
        self.linear1 = _Linear(768, 3072)
        self.linear2 = _Linear(3072, 768)
        self.norm1 = _Norm(768)
        self.norm2 = _Norm(768)


class _FeatureExtractor(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv0 = _Conv(1, 512, 10)
        self.norm0 = _Norm(512)
        for i, k in enumerate((3, 3, 3, 3, 2, 2)):
            setattr(self, f"conv{i + 1}", _Conv(512, 512, k))


class _FeatureProjection(nn.Module):
    def __init__(self):
        super().__init__()
        self.norm = _Norm(512)
        self.projection = _Linear(512, 768)


class _PositionalEmbedding(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = _WeightNormConv()


class _Encoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.layers = nn.ModuleList([_Layer() for _ in range(12)])


class _DeviceEncoder(nn.Module):
    """What the two encoders share on the host: the weight table, the (B, 1, T) check, the ragged counts.  A subclass names
    itself (`_NAME`), its weight struct and tensors (`_STRUCT`, `_named_tensors`), its frame rule (`_frames`: T -> frames, 0
    when too short) and its check of ragged counts (`_check_n_samples`)."""
    _NAME = _STRUCT = _frames = _check_n_samples = None

    def _make_table(self):
        self._table = hipddsp.WeightTable(self._STRUCT, type(self)._named_tensors, self._NAME)

    def rebind(self):
        """Forget the weight struct and have the library re-prepare the weights: after a submodule was replaced, or after a
        write `_version` does not count (`hipddsp.WeightTable`)."""
        self._table.invalidate()

    def _weights_struct(self):
        return self._table.struct(self)[0]

    @classmethod
    def frames(cls, T):
        """Encoder frames of T samples at 16 kHz; ValueError when the audio is too short for the conv stack."""
        n = cls._frames(int(T))
        if n <= 0:
            raise ValueError(f"{cls._NAME}: {int(T)} samples are too short for the conv stack")
        return n

    def _wav(self, wav):
        if not wav.is_cuda:
            raise RuntimeError(f"{self._NAME} runs on a HIP device only (no CPU fallback)")
        if wav.dim() != 3 or wav.shape[1] != 1:
            raise ValueError(f"{self._NAME}: wav must be (B, 1, T)")
        self.frames(wav.shape[-1])
        return wav[:, 0].contiguous().float()

    @classmethod
    def counts(cls, n_samples, B, T, device):
        """`n_samples` of a ragged (B, 1, T) batch, checked on the host and uploaded once -> `RaggedCounts`."""
        vals = cls._check_n_samples(n_samples, B, T)
        return RaggedCounts(vals, T, hipddsp.context_for(device).ragged_counts(vals))

    @classmethod
    def _counts(cls, wav, n_samples):
        """`n_samples` checked on the host (ValueError before anything is launched) -> its (B,) int32 device tensor, or None."""
        if n_samples is None:
            return None
        if wav.dim() != 3 or wav.shape[1] != 1:
            raise ValueError(f"{cls._NAME}: wav must be (B, 1, T)")
        if isinstance(n_samples, RaggedCounts):
            if len(n_samples.values) != wav.shape[0] or n_samples.T != wav.shape[-1] or n_samples.dev.device != wav.device:
                raise ValueError(f"{cls._NAME}: these RaggedCounts were made for another batch shape or device")
            return n_samples.dev
        vals = cls._check_n_samples(n_samples, wav.shape[0], wav.shape[-1])
        if not wav.is_cuda:
            raise RuntimeError(f"{cls._NAME} runs on a HIP device only (no CPU fallback)")
        return hipddsp.context_for(wav.device).ragged_counts(vals)


class HubertSoft(_DeviceEncoder):
    _NAME, _STRUCT = "HubertSoft", hipddsp.HubertWeights
    _frames = staticmethod(lambda T: hipddsp.hubert_frames(T))
    _check_n_samples = staticmethod(lambda n, B, T: hipddsp.check_hubert_n_samples(n, B, T))

    def __init__(self):
        super().__init__()
        self.masked_spec_embed = nn.Parameter(torch.zeros(768))
        self.feature_extractor = _FeatureExtractor()
        self.feature_projection = _FeatureProjection()
        self.positional_embedding = _PositionalEmbedding()
        self.norm = _Norm(768)
        self.encoder = _Encoder()
        self.proj = _Linear(768, 256)
        self.label_embedding = nn.Embedding(100, 256)
        self._make_table()

    # ---- pointer table ---------------------------------------------------------------------------
    def _named_tensors(self):
        """(HubertWeights field, tensor) in the order of `ddsp_hubert_weights`."""
        fe, fp, pc = self.feature_extractor, self.feature_projection, self.positional_embedding.conv
        out = [("conv0_w", fe.conv0.weight), ("norm0_w", fe.norm0.weight), ("norm0_b", fe.norm0.bias)]
        out += [(f"conv{i}_w", getattr(fe, f"conv{i}").weight) for i in range(1, 7)]
        out += [("fp_norm_w", fp.norm.weight), ("fp_norm_b", fp.norm.bias), ("fp_proj_w", fp.projection.weight),
                ("fp_proj_b", fp.projection.bias), ("pos_b", pc.bias), ("pos_g", pc.weight_g), ("pos_v", pc.weight_v),
                ("norm_w", self.norm.weight), ("norm_b", self.norm.bias)]
        for i, ly in enumerate(self.encoder.layers):
            t = (ly.self_attn.in_proj_weight, ly.self_attn.in_proj_bias, ly.self_attn.out_proj.weight,
                 ly.self_attn.out_proj.bias, ly.linear1.weight, ly.linear1.bias, ly.linear2.weight, ly.linear2.bias,
                 ly.norm1.weight, ly.norm1.bias, ly.norm2.weight, ly.norm2.bias)
            out += [(f"l{i}_{n}", x) for n, x in zip(hipddsp.HUBERT_LAYER_FIELDS, t)]
        out += [("proj_w", self.proj.weight), ("proj_b", self.proj.bias)]
        return out

    @torch.no_grad()
    def units(self, wav, n_samples=None):
        """:: (B, 1, T) 16 kHz -> (B, Frame, 256).  `n_samples` (a sequence of B ints or a CPU integer tensor (B,), 1 <=
        n_samples[b] <= T, each long enough for the conv stack): a RAGGED batch.  Row b is then, over its own
        `n_frames(n_samples[b])` frames, what `units(wav[b:b+1, :, :n_samples[b]])` returns, and exactly 0 after them; the
        samples past a row's count may hold anything (they are replaced by selection, never multiplied by a mask)."""
        n_dev = self._counts(wav, n_samples)
        x = self._wav(wav)
        return hipddsp.context_for(x.device).hubert_units(self._weights_struct(), x, n_dev)

    @torch.no_grad()
    def encode(self, wav, layer=None, n_samples=None):
        """:: (B, 1, T) -> the hidden state (B, Frame, 768) after `layer` transformer layers (all 12 when None), or the conv
        stack's output (B, Frame, 512) for layer=-1.  Unlike the reference's `encode`, the audio is padded here as `units`
        pads it, and no mask is returned.  `n_samples`: ragged batch, as in `units`."""
        layer = 12 if layer is None else int(layer)
        if not -1 <= layer <= 12:
            raise ValueError("HubertSoft.encode: layer in -1..12")
        n_dev = self._counts(wav, n_samples)
        x = self._wav(wav)
        return hipddsp.context_for(x.device).hubert_encode(self._weights_struct(), x, layer, n_dev)

    def forward(self, wav, n_samples=None):
        return self.units(wav, n_samples)


# ---- the HuBERT-base form of fairseq ------------------------------------------------------------------------------------

class _Slots(nn.Module):
    """A module whose children sit under the given names: fairseq's `nn.Sequential` indices, with the gaps its dropout and
    activation entries leave (`conv_layers.0.2` is the GroupNorm)."""

    def __init__(self, **children):
        super().__init__()
        for name, child in children.items():
            self.add_module(name.lstrip("_"), child)

    def __getitem__(self, i):
        return getattr(self, str(i))


class _BaseAttention(nn.Module):
    def __init__(self):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (_Linear(768, 768) for _ in range(4))


class _BaseLayer(nn.Module):
    """fairseq's `TransformerSentenceEncoderLayer` (post-norm: `layer_norm_first=False`)."""

    def __init__(self):
        super().__init__()
        self.self_attn = _BaseAttention()
        self.self_attn_layer_norm = _Norm(768)
        self.fc1 = _Linear(768, 3072)
        self.fc2 = _Linear(3072, 768)
        self.final_layer_norm = _Norm(768)


class _BaseFeatureExtractor(nn.Module):
    def __init__(self):
        super().__init__()
        first = _Slots(_0=_Conv(1, 512, 10), _2=_Norm(512))
        self.conv_layers = nn.ModuleList([first] + [_Slots(_0=_Conv(512, 512, k)) for k in (3, 3, 3, 3, 2, 2)])


class _BaseEncoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.pos_conv = _Slots(_0=_WeightNormConv())
        self.layers = nn.ModuleList([_BaseLayer() for _ in range(12)])
        self.layer_norm = _Norm(768)


def load_fairseq_state(obj):
    """What `torch.load` returned for a fairseq HuBERT checkpoint -> its state dict: `obj` is the state dict itself or holds it
    under "model"; a `module.` prefix (DataParallel) is stripped."""
    sd = obj.get("model") if isinstance(obj, dict) and isinstance(obj.get("model"), dict) else obj
    if not isinstance(sd, dict) or not sd or not all(isinstance(v, torch.Tensor) for v in sd.values()):
        raise ValueError("load_fairseq_state: expected a state dict of tensors, or a dict holding one under 'model'")
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}


def read_fairseq_checkpoint(path):
    """path -> the state dict (`load_fairseq_state`).  The file is read with `weights_only=True` first; a file that holds more
    than tensors is read again without it, and when that needs fairseq or omegaconf (a checkpoint as fairseq's trainer wrote
    it carries its config objects) the RuntimeError says how to make a plain file."""
    try:
        obj = torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError:
        try:
            obj = torch.load(path, map_location="cpu", weights_only=False)
        except (ImportError, AttributeError) as e:
            raise RuntimeError(
                f"{path}: this checkpoint carries fairseq / omegaconf objects beside its weights ({e}), and neither package "
                "is installed or needed here.  Save the weights once as a plain state dict on a machine that has fairseq: "
                "ckpt = torch.load(path, weights_only=False); torch.save(ckpt['model'], 'plain.pt') - and pass that file") from e
    return load_fairseq_state(obj)


class HubertBase(_DeviceEncoder):
    """fairseq's `HubertModel` in the base architecture, for inference: `units` is `extract_features(source, padding_mask =
    all False, output_layer=layer)`, with `project` followed by `final_proj`.  `mask_emb` and `label_embs_concat` are in the
    state dict and never read; `label_embs_concat` takes whatever first dimension a checkpoint has (`load_state_dict`)."""
    _NAME, _STRUCT = "HubertBase", hipddsp.HubertBaseWeights
    _frames = staticmethod(lambda T: hipddsp.hubert_base_frames(T))
    _check_n_samples = staticmethod(lambda n, B, T: hipddsp.check_hubert_base_n_samples(n, B, T))

    def __init__(self):
        super().__init__()
        self.mask_emb = nn.Parameter(torch.zeros(768))
        self.label_embs_concat = nn.Parameter(torch.zeros(504, 256))
        self.feature_extractor = _BaseFeatureExtractor()
        self.post_extract_proj = _Linear(512, 768)
        self.encoder = _BaseEncoder()
        self.layer_norm = _Norm(512)
        self.final_proj = _Linear(768, 256)
        self._make_table()

    def load_state_dict(self, state_dict, *args, **kwargs):
        t = state_dict.get("label_embs_concat")
        if isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape != self.label_embs_concat.shape:
            own = self.label_embs_concat
            self.label_embs_concat = nn.Parameter(torch.zeros(t.shape, dtype=own.dtype, device=own.device))
        return super().load_state_dict(state_dict, *args, **kwargs)

    def _named_tensors(self):
        """(HubertBaseWeights field, tensor)."""
        cl, enc, pc = self.feature_extractor.conv_layers, self.encoder, self.encoder.pos_conv[0]
        out = [("conv0_w", cl[0][0].weight), ("norm0_w", cl[0][2].weight), ("norm0_b", cl[0][2].bias)]
        out += [(f"conv{i}_w", cl[i][0].weight) for i in range(1, 7)]
        out += [("fp_norm_w", self.layer_norm.weight), ("fp_norm_b", self.layer_norm.bias),
                ("fp_proj_w", self.post_extract_proj.weight), ("fp_proj_b", self.post_extract_proj.bias),
                ("pos_b", pc.bias), ("pos_g", pc.weight_g), ("pos_v", pc.weight_v),
                ("norm_w", enc.layer_norm.weight), ("norm_b", enc.layer_norm.bias)]
        for i, ly in enumerate(enc.layers):
            at = ly.self_attn
            t = (at.q_proj.weight, at.q_proj.bias, at.k_proj.weight, at.k_proj.bias, at.v_proj.weight, at.v_proj.bias,
                 at.out_proj.weight, at.out_proj.bias, ly.self_attn_layer_norm.weight, ly.self_attn_layer_norm.bias,
                 ly.fc1.weight, ly.fc1.bias, ly.fc2.weight, ly.fc2.bias, ly.final_layer_norm.weight, ly.final_layer_norm.bias)
            out += [(f"l{i}_{n}", x) for n, x in zip(hipddsp.HUBERT_BASE_LAYER_FIELDS, t)]
        out += [("proj_w", self.final_proj.weight), ("proj_b", self.final_proj.bias)]
        return out

    @torch.no_grad()
    def units(self, wav, n_samples=None, layer=9, project=True):
        """:: (B, 1, T) 16 kHz, not padded -> (B, Frame, 256) with `project`, else the hidden state (B, Frame, 768) after
        `layer` (1..12) transformer layers.  `n_samples`: a RAGGED batch as in `HubertSoft.units`, under this encoder's frame
        rule (`frames`: 400 samples give the first frame)."""
        layer = int(layer)
        if not 1 <= layer <= 12:
            raise ValueError("HubertBase.units: layer in 1..12")
        n_dev = self._counts(wav, n_samples)
        x = self._wav(wav)
        return hipddsp.context_for(x.device).hubert_base_units(self._weights_struct(), x, layer, bool(project), n_dev)

    def forward(self, wav, n_samples=None):
        return self.units(wav, n_samples)
