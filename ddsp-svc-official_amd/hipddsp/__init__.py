"""ctypes binding of libddsp_amd.so (the C ABI declared in include/ddsp_amd.h).

PyTorch is used only for device memory and streams: every call passes raw device pointers and the
current HIP stream.  There is NO CPU fallback: without the shared library or without a GPU the
calls raise.
"""
import ctypes
import math as _math
import numbers
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libddsp_amd.so")

DDSP_OK, DDSP_ERR_ARG, DDSP_ERR_HIP, DDSP_ERR_OOM = 0, -1, -2, -3

COMB_NONE, COMB_SINC, COMB_SINC_GATED = 0, 1, 2
FIR_ALLPASS, FIR_DYNAMIC, FIR_STATIC = 0, 1, 2
EXC_AUDIO, EXC_UNIT_NOISE, EXC_GENERATE = 0, 1, 2
FIR_FP32, FIR_SPLIT_BF16 = 0, 3   # ddsp_ltv_fir `math` (include/ddsp_amd.h)
ABI_VERSION = 8                   # DDSP_ABI_VERSION of include/ddsp_amd.h (struct layouts: U2CWeights, HubertWeights, CrepeWeights)
MATH_FP32, MATH_SPLIT_BF16 = 0, 3  # ddsp_ctx_set_math
ATTENTION_CAUSAL = 200            # ddsp_performer_attention: causal_linear_attention (pcmer.py:170-188)
SLICER_PAD = {"constant": 0, "reflect": 1}   # ddsp_slicer `pad_mode`: librosa >= 0.10 / older librosa
ATTENTION_PAIR = 100              # ddsp_performer_attention: the split-bf16 key / query kernel pair instead of the fused kernel

_c = ctypes
_vp, _i64, _u64, _int, _f32, _f64 = _c.c_void_p, _c.c_int64, _c.c_uint64, _c.c_int, _c.c_float, _c.c_double


class U2CWeights(_c.Structure):
    """Mirror of `ddsp_u2c_weights` (include/ddsp_amd.h): device pointers into the state dict."""
    _fields_ = (
        [(n, _vp) for n in ("prenet_conv1_w", "prenet_conv1_b", "prenet_gn_w", "prenet_gn_b",
                            "prenet_conv2_w", "prenet_conv2_b",
                            "f0_w", "f0_b", "phase_w", "phase_b", "volume_w", "volume_b", "spk_table")]
        + [("n_spk", _int), ("n_unit", _int), ("n_out", _int), ("causal", _int)]
        + [(f"l{i}_{n}", _vp) for i in range(3) for n in (
            "norm_w", "norm_b", "q_w", "q_b", "k_w", "k_b", "v_w", "v_b", "proj", "out_w", "out_b",
            "cm_ln_w", "cm_ln_b", "cm_pw1_w", "cm_pw1_b", "cm_dw_w", "cm_dw_b", "cm_pw2_w", "cm_pw2_b")]
        + [(n, _vp) for n in ("final_ln_w", "final_ln_b", "head_g", "head_v", "head_b")]
        + [("version", _c.c_uint64)]     # change counter of the weight values (0: prepare the weights on every call)
    )


HUBERT_LAYER_FIELDS = ("in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "linear1_w", "linear1_b", "linear2_w",
                       "linear2_b", "norm1_w", "norm1_b", "norm2_w", "norm2_b")


class HubertWeights(_c.Structure):
    """Mirror of `ddsp_hubert_weights` (include/ddsp_amd.h): device pointers into the HubertSoft state dict."""
    _fields_ = (
        [(n, _vp) for n in ("conv0_w", "norm0_w", "norm0_b")]
        + [(f"conv{i + 1}_w", _vp) for i in range(6)]
        + [(n, _vp) for n in ("fp_norm_w", "fp_norm_b", "fp_proj_w", "fp_proj_b", "pos_b", "pos_g", "pos_v", "norm_w", "norm_b")]
        + [(f"l{i}_{n}", _vp) for i in range(12) for n in HUBERT_LAYER_FIELDS]
        + [(n, _vp) for n in ("proj_w", "proj_b")]
        + [("version", _c.c_uint64)]     # change counter of the weight values (0: prepare the weights on every call)
    )


HUBERT_BASE_LAYER_FIELDS = ("q_w", "q_b", "k_w", "k_b", "v_w", "v_b", "out_w", "out_b", "ln1_w", "ln1_b", "fc1_w", "fc1_b",
                            "fc2_w", "fc2_b", "ln2_w", "ln2_b")


class HubertBaseWeights(_c.Structure):
    """Mirror of `ddsp_hubert_base_weights` (include/ddsp_amd.h): device pointers into a fairseq HubertModel state dict."""
    _fields_ = (
        [(n, _vp) for n in ("conv0_w", "norm0_w", "norm0_b")]
        + [(f"conv{i + 1}_w", _vp) for i in range(6)]
        + [(n, _vp) for n in ("fp_norm_w", "fp_norm_b", "fp_proj_w", "fp_proj_b", "pos_b", "pos_g", "pos_v", "norm_w", "norm_b")]
        + [(f"l{i}_{n}", _vp) for i in range(12) for n in HUBERT_BASE_LAYER_FIELDS]
        + [(n, _vp) for n in ("proj_w", "proj_b")]
        + [("version", _c.c_uint64)]     # change counter of the weight values (0: prepare the weights on every call)
    )


class CrepeWeights(_c.Structure):
    """Mirror of `ddsp_crepe_weights` (include/ddsp_amd.h): device pointers into a CREPE state dict (torchcrepe's keys) and the
    output channels of its six convolutions."""
    _fields_ = (
        [(f"{n}{i + 1}_{s}", _vp) for n, s in (("conv", "w"), ("conv", "b"), ("bn", "w"), ("bn", "b"), ("bn", "mean"),
                                                 ("bn", "var")) for i in range(6)]
        + [("cls_w", _vp), ("cls_b", _vp)]
        + [("width", _int * 6)]
        + [("version", _c.c_uint64)]     # change counter of the weight values (0: prepare the weights on every call)
    )


class WeightTable:
    """The weight struct (U2CWeights, HubertWeights, HubertBaseWeights) of one model, built from `named_tensors(module)` -> [(field, tensor)].

    The library keeps the weights it prepares from the struct while its pointers, integers and `version` stand.  `version` is
    a per-model nonce (two models whose tensors the allocator placed at the same addresses differ in it) plus the sum of
    the tensors' `_version` counters, so every write torch counts re-prepares them: an in-place op, `load_state_dict`, an
    optimizer step (`training.AdamW` calls `torch.autograd.graph.increment_version`).  A write torch does not count - into
    `p.data`, or a foreign kernel writing through the pointer - needs `invalidate()` or `increment_version(p)`.

    `copy`: a tensor that is not contiguous fp32 is passed as a contiguous fp32 copy (and the struct is not kept); otherwise
    it raises.  `grad_uncached`: in grad mode `version` is 0 (prepare on every call).  `ints`: the struct's integer fields."""

    def __init__(self, struct_cls, named_tensors, owner, copy=False, grad_uncached=False, **ints):
        self.struct_cls, self.named_tensors, self.owner = struct_cls, named_tensors, owner
        self.copy, self.grad_uncached, self.ints = copy, grad_uncached, ints
        self.invalidate()

    def invalidate(self):
        """Forget the tensor slots and the struct, and draw a new nonce: the next call re-reads the module (after a submodule
        was replaced) and the library re-prepares the weights."""
        self._slots = self._ws = None
        self._nonce = int.from_bytes(os.urandom(6), "little") << 16

    def struct(self, module):
        """-> (struct, the tensors it points into: hold them until the call has been queued)."""
        if self._slots is None:
            # (field, owning dict, key), built once: reading `d[k]` costs a dict lookup where `module.weight` goes through
            # nn.Module.__getattr__.  A Parameter replaced by setattr lands in the same dict and is seen.
            by_id = {id(t): (d, k) for mod in module.modules() for d in (mod._parameters, mod._buffers)
                     for k, t in d.items() if t is not None}
            self._slots = [(name,) + by_id[id(t)] for name, t in self.named_tensors(module)]
        tensors = [d[k] for _, d, k in self._slots]
        uncached = self.grad_uncached and torch.is_grad_enabled()
        key = (uncached,) + tuple([(t.data_ptr(), t._version) for t in tensors])
        if self._ws is not None and self._ws[0] == key:
            return self._ws[1], self._ws[2]
        w = self.struct_cls(**self.ints)
        keep = []
        for (name, _, _), t in zip(self._slots, tensors):
            if not t.is_cuda:
                raise RuntimeError(f"{self.owner} parameters must live on a HIP device (no CPU fallback)")
            t = t.detach()
            if not t.is_contiguous() or t.dtype != torch.float32:
                if not self.copy:
                    raise ValueError(f"{self.owner} parameters must be contiguous fp32")
                t = t.contiguous().float()
            keep.append(t)
            setattr(w, name, t.data_ptr())
        w.version = 0 if uncached else (self._nonce + 1 + sum(int(t._version) for t in tensors)) & ((1 << 64) - 1)
        # (a copy has a new address every time: such a struct is not worth keeping)
        if all(a.data_ptr() == b.data_ptr() for a, b in zip(keep, tensors)):
            self._ws = (key, w, keep)
        return w, keep


class DatasetView(_c.Structure):
    """Mirror of `ddsp_dataset_view` (include/ddsp_amd.h): device pointers to a packed dataset's arenas and per-file tables."""
    _fields_ = ([(n, _vp) for n in ("audio", "units", "f0", "volume", "audio_off", "audio_len", "frame_off", "frames",
                                    "spk_id", "duration", "next_valid")]
                + [("n_files", _i64), ("total_frames", _i64)]
                + [(n, _c.c_int32) for n in ("n_aunit", "n_unit", "hop", "sample_rate", "fp16")])


class FirProblem(_c.Structure):
    """Mirror of `ddsp_fir_problem`."""
    _fields_ = [("mode", _int), ("col", _int), ("n_mag", _int), ("f0_frames", _vp), ("ir", _vp)]


class ProfEntry(_c.Structure):
    """Mirror of `ddsp_prof_entry`."""
    _fields_ = [("family", _int), ("name", _c.c_char * 36), ("launches", _i64), ("ms_total", _c.c_double),
                ("flops_total", _c.c_double), ("bytes_total", _c.c_double)]


CONV_X_SPLIT, CONV_ACT_SPLIT = 1, 2


def presplit(w):
    """fp32 matrix (rows, K), K % 8 == 0 -> the same bytes-per-row with every group of 8 values replaced by their 8 bf16 high
    parts and 8 bf16 remainders (round to nearest even, twice): the pre-split operand layout of the split-bf16 GEMM
    (gemm::Args::B_split / A_split), bit-identical to what the kernels produce when they split in the loop."""
    if w.dtype != torch.float32 or w.shape[-1] % 8:
        raise ValueError("presplit: fp32 with a multiple of 8 columns")
    g = w.contiguous().reshape(*w.shape[:-1], w.shape[-1] // 8, 8)
    hi = g.to(torch.bfloat16)
    lo = (g - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, lo], dim=-1).contiguous().view(torch.float32).reshape(w.shape)


FAMILIES = ["phase_scan", "fir_act", "fir_dft_gemm", "ltv_fir", "u2c_prep", "u2c_gemm_conv3", "u2c_gemm_linear",
            "u2c_gemm_feat", "u2c_gemm_ctx", "u2c_gemm_attnout", "u2c_rowwise", "sins_bank", "spectral_ola", "rss_loss",
            "sola", "upsample", "other", "ltv_fir_bwd", "fir_synth_bwd", "u2c_bwd", "optim"]

# name -> (restype, argtypes); every symbol declared in include/ddsp_amd.h must be listed here
SIGNATURES = {
    "ddsp_abi_version": (_int, []),
    "ddsp_ctx_create": (_int, [_c.POINTER(_vp), _int]),
    "ddsp_ctx_destroy": (_int, [_vp]),
    "ddsp_last_error": (_c.c_char_p, [_vp]),
    "ddsp_ctx_reserve": (_int, [_vp, _u64]),
    "ddsp_ctx_poll_error": (_int, [_vp]),
    "ddsp_ctx_set_math": (_int, [_vp, _int]),
    "ddsp_ctx_get_math": (_int, [_vp]),
    "ddsp_upsample": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _int, _vp]),
    "ddsp_phase_scan": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "ddsp_fir_from_ctrl": (_int, [_vp, _vp, _int, _vp, _i64, _int, _vp, _i64, _int, _vp]),
    "ddsp_fir_from_ctrl_group": (_int, [_vp, _vp, _vp, _i64, _i64, _int, _vp, _int]),
    "ddsp_ltv_fir_bwd": (_int, [_vp, _vp, _vp, _int, _u64, _vp, _vp, _i64, _i64, _int, _int, _vp, _vp]),
    "ddsp_fir_from_ctrl_bwd": (_int, [_vp, _vp, _int, _vp, _i64, _int, _vp, _i64, _int, _vp, _vp, _i64]),
    "ddsp_sins_bank": (_int, [_vp, _vp, _vp, _i64, _int, _vp, _vp, _i64, _i64, _int, _int, _vp]),
    "ddsp_spectral_ola": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _int, _u64, _i64, _i64, _int, _vp]),
    "ddsp_sins_bank_bwd": (_int, [_vp, _vp, _vp, _i64, _int, _vp, _vp, _vp, _i64, _i64, _int, _int, _vp, _i64]),
    "ddsp_spectral_ola_bwd": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _int, _u64, _vp, _i64, _i64, _int, _vp, _i64]),
    "ddsp_rss_loss": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _c.POINTER(_int), _vp, _c.POINTER(_int), _i64, _c.POINTER(_int),
                             _c.POINTER(_int), _int, _f32, _f32, _vp, _vp]),
    "ddsp_sola": (_int, [_vp, _vp, _vp, _int, _i64, _int, _int, _int, _int, _vp, _vp, _vp]),
    "ddsp_volume_gate": (_int, [_vp, _vp, _vp, _vp, _f32, _i64, _i64, _int]),
    "ddsp_volume_gate_rows": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _i64, _i64, _i64, _int]),
    "ddsp_volume_gate_files": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _f32, _i64, _i64, _i64, _int]),
    "ddsp_pieces_gather": (_int, [_vp] * 8 + [_i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "ddsp_pieces_gather_jobs": (_int, [_vp] * 8 + [_i64, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "ddsp_pieces_gather_keys": (_int, [_vp] * 9 + [_i64, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "ddsp_stitch": (_int, [_vp, _vp, _vp, _i64, _vp, _i64]),
    "ddsp_pcm16": (_int, [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    "ddsp_phase_vocoder": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp]),
    "ddsp_volume_extract": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _int, _vp]),
    "ddsp_volume_extract_frac": (_int, [_vp, _vp, _vp, _i64, _i64, _f64, _vp]),
    "ddsp_align_units": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _vp]),
    "ddsp_gemm_res_ln": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp, _vp, _int]),
    "ddsp_u2c_dwconv_pw2": (_int, [_vp] * 11 + [_int, _int, _int, _int, _vp, _vp, _vp]),
    "ddsp_conv1d_pair_supported": (_int, [_vp, _int, _int, _int]),
    "ddsp_conv1d_pair": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _int, _f32, _vp, _vp, _vp, _int]),
    "ddsp_retime_f0": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _f64, _f64, _f32, _f64, _i64, _vp, _vp]),
    "ddsp_resample_length": (_i64, [_i64, _int, _int]),
    "ddsp_resample": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _int, _int, _int, _vp]),
    "ddsp_conv1d": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _int, _int, _f32, _vp, _vp, _vp, _f32, _vp, _int,
                           _vp, _int]),
    "ddsp_nsf_source": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _f32, _vp, _vp]),
    "ddsp_nsf_noise_conv": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _int, _int, _int, _int, _i64, _vp]),
    "ddsp_nsf_post": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _f32, _vp, _vp, _int]),
    "ddsp_nsf_mean": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _i64, _vp, _vp, _f32, _int]),
    "ddsp_log_mel": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _f32, _vp]),
    "ddsp_adamw_step": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _i64]),
    "ddsp_adamw_step_multi": (_int, [_vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _f32, _i64, _f32]),
    "ddsp_gemm_f32": (_int, [_vp, _vp, _vp, _i64, _int, _vp, _i64, _int, _vp, _vp, _i64, _int, _int, _int, _int, _int]),
    "ddsp_performer_attention": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _int]),
    "ddsp_hubert_frames": (_i64, [_i64]),
    "ddsp_hubert_soft_units": (_int, [_vp, _vp, _c.POINTER(HubertWeights), _vp, _i64, _i64, _vp, _vp]),
    "ddsp_hubert_encode": (_int, [_vp, _vp, _c.POINTER(HubertWeights), _vp, _i64, _i64, _vp, _int, _vp]),
    "ddsp_hubert_base_frames": (_i64, [_i64]),
    "ddsp_hubert_base_units": (_int, [_vp, _vp, _c.POINTER(HubertBaseWeights), _vp, _i64, _i64, _vp, _int, _int, _vp]),
    "ddsp_softmax_attention": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _vp, _int, _vp]),
    "ddsp_stft_frames": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _int, _int, _i64, _vp]),
    "ddsp_retime_f0_keyed": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _f64, _vp, _int, _vp, _vp, _f64, _i64, _vp, _vp]),
    "ddsp_enhancer_keys": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp]),
    "ddsp_resample_keyed_plan": (_int, [_vp, _vp, _int, _c.POINTER(_int), _c.POINTER(_int), _int, _c.POINTER(_vp)]),
    "ddsp_resample_keyed_plan_destroy": (None, [_vp]),
    "ddsp_resample_keyed_length": (_i64, [_vp, _i64]),
    "ddsp_resample_keyed": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
    "ddsp_crepe_frames": (_i64, [_i64, _int]),
    "ddsp_crepe_activations": (_int, [_vp, _vp, _c.POINTER(CrepeWeights), _vp, _i64, _i64, _vp, _vp, _i64, _int, _vp]),
    "ddsp_crepe_decode": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _f32, _f32, _i64, _u64, _vp, _int, _vp, _vp, _vp]),
    "ddsp_stream_push": (_int, [_vp, _vp, _vp, _int, _i64, _vp, _i64]),
    "ddsp_bank_gather": (_int, [_vp, _vp, _vp, _int, _int, _vp, _i64, _vp, _i64, _vp, _vp, _int, _vp, _vp, _vp, _int, _vp, _vp, _vp,
                                _vp, _vp, _vp]),
    "ddsp_bank_scatter": (_int, [_vp, _vp, _vp, _int, _int, _vp, _int, _vp]),
    "ddsp_bank_glide": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _vp, _int, _vp, _int, _i64, _i64, _i64, _f64, _vp]),
    "ddsp_bank_key_glide": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp, _int, _vp, _i64, _i64, _i64, _f64, _vp]),
    "ddsp_ctrl_warp": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _int, _vp, _int, _i64, _vp, _i64, _vp]),
    "ddsp_f0_tune": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp]),
    "ddsp_units_retrieve": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _int,
                                   _vp, _i64, _vp, _vp]),
    "ddsp_units_retrieve_workspace": (_int, [_vp, _i64, _i64, _int, _i64, _vp]),
    "ddsp_envelope_rms": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _int, _i64, _vp, _vp]),
    "ddsp_envelope_apply": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp,
                                   _i64, _vp, _vp, _vp, _i64]),
    "ddsp_units_index_norms": (_int, [_vp, _vp, _vp, _i64, _i64, _vp]),
    "ddsp_units_kmeans_assign": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
    "ddsp_units_kmeans_update": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _int, _vp, _vp, _vp, _i64]),
    "ddsp_bank_features_gather": (_int, [_vp, _vp, _vp, _int, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp,
                                         _vp, _vp, _vp, _vp]),
    "ddsp_bank_signal_scatter": (_int, [_vp, _vp, _vp, _int, _int, _vp, _i64, _vp]),
    "ddsp_f0_postfilter": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _int, _f64, _i64, _i64, _vp, _f32, _int, _f32, _vp]),
    "ddsp_f0_ac_frames": (_i64, [_i64, _int, _f64, _f64]),
    "ddsp_f0_ac": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _int, _f64, _f64, _f64, _i64, _i64, _int, _vp, _vp]),
    "ddsp_slicer_frames": (_i64, [_i64, _i64, _i64]),
    "ddsp_slicer": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _f64, _i64, _i64, _i64, _int, _vp, _vp, _vp, _i64]),
    "ddsp_profile_begin": (_int, [_vp, _u64]),
    "ddsp_profile_mask": (_int, [_vp, _u64]),
    "ddsp_profile_end": (_int, [_vp, _c.POINTER(ProfEntry), _int, _c.POINTER(_int)]),
    "ddsp_unit2ctrl_fwd": (_int, [_vp, _vp, _c.POINTER(U2CWeights), _vp, _vp, _vp, _vp, _vp, _i64,
                                  _c.POINTER(_i64), _c.POINTER(_f32), _int, _i64, _i64, _vp, _vp]),
    "ddsp_unit2ctrl_bwd": (_int, [_vp, _vp, _c.POINTER(U2CWeights), _vp, _vp, _vp, _vp, _vp, _i64,
                                  _c.POINTER(_i64), _c.POINTER(_f32), _int, _i64, _i64, _vp, _vp, _c.POINTER(U2CWeights), _vp]),
    "ddsp_unit2ctrl_fwd_rowmix": (_int, [_vp, _vp, _c.POINTER(U2CWeights), _vp, _vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _vp, _vp]),
    "ddsp_unit2ctrl_fwd_framemix": (_int, [_vp, _vp, _c.POINTER(U2CWeights), _vp, _vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _vp, _vp]),
    "ddsp_mix_timeline": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _int, _i64, _vp, _vp]),
    "ddsp_ragged_frames": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _int, _vp]),
    "ddsp_ragged_crop": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int]),
    "ddsp_ragged_noise": (_int, [_vp, _vp, _vp, _u64, _vp, _i64, _i64, _int, _vp]),
    "ddsp_ltv_fir": (_int, [_vp, _vp, _vp, _int, _u64, _vp, _i64, _i64, _int, _int, _vp, _vp, _vp, _int]),
    "ddsp_unit2ctrl_keep_bytes": (_i64, [_c.POINTER(U2CWeights), _i64, _i64]),
    "ddsp_unit2ctrl_fwd_keep": (_int, [_vp, _vp, _c.POINTER(U2CWeights), _vp, _vp, _vp, _vp, _vp, _i64,
                                       _c.POINTER(_i64), _c.POINTER(_f32), _int, _i64, _i64, _vp, _vp, _i64, _vp]),
    "ddsp_unit2ctrl_bwd_kept": (_int, [_vp, _vp, _c.POINTER(U2CWeights), _vp, _vp, _vp, _vp, _vp, _i64,
                                       _c.POINTER(_i64), _c.POINTER(_f32), _int, _i64, _i64, _vp, _vp, _i64, _vp,
                                       _c.POINTER(U2CWeights)]),
    "ddsp_ragged_frames_adjoint": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64]),
    "ddsp_rss_loss_rows": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _c.POINTER(_int), _vp, _c.POINTER(_int), _c.POINTER(_int),
                                  _int, _f32, _f32, _vp]),
    "ddsp_vc_f0_map": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _vp, _vp, _vp]),
    "ddsp_dataset_gather": (_int, [_vp, _vp, _c.POINTER(DatasetView), _vp, _vp, _i64, _i64, _u64, _vp, _i64, _f64, _i64, _i64,
                                   _vp, _vp, _vp, _vp, _vp, _vp]),
}

_lib = None
_lib_lock = threading.Lock()


def load_library():
    """Loads libddsp_amd.so from the package tree; raises if it has not been built."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"{LIB_PATH} is missing: build it with `python ddsp-svc-official_amd/hipddsp/build.py` "
                    "(there is no CPU fallback for the synthesis path)")
            lib = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)   # AttributeError if the symbol is not exported
                fn.restype = res
                fn.argtypes = args
            if lib.ddsp_abi_version() != ABI_VERSION:
                raise RuntimeError(f"{LIB_PATH} has ABI version {lib.ddsp_abi_version()}, this binding needs {ABI_VERSION}: "
                                   "rebuild it (`python ddsp-svc-official_amd/hipddsp/build.py`)")
            _lib = lib
    return _lib


def _check_counts(name, counts, B):
    """A ragged batch's per-row counts as a list of B Python ints (a host check; the callers check the range)."""
    if isinstance(counts, torch.Tensor):
        if counts.is_cuda:
            raise ValueError(f"{name} must be a CPU tensor or a sequence of ints (it is checked on the host)")
        if counts.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) or counts.dim() != 1:
            raise ValueError(f"{name} must be an integer tensor of shape (B,), got {counts.dtype} {tuple(counts.shape)}")
        vals = counts.tolist()
    else:
        try:
            vals = list(counts)
        except TypeError:
            raise ValueError(f"{name} must be a sequence of B ints or a CPU integer tensor of shape (B,)") from None
        for v in vals:
            if isinstance(v, bool) or not isinstance(v, numbers.Integral):
                raise ValueError(f"{name} must hold ints, got {type(v).__name__} {v!r}")
        vals = [int(v) for v in vals]
    if len(vals) != int(B):
        raise ValueError(f"{name} must hold B={int(B)} counts, got {len(vals)}")
    return vals


def check_n_frames(n_frames, B, Fr):
    """The per-row frame counts of a ragged batch as a list of B Python ints, 1 <= n <= Fr; anything else raises ValueError
    (a host check: nothing is launched).  Accepted: a sequence of ints, or a CPU integer tensor of shape (B,)."""
    vals = _check_counts("n_frames", n_frames, B)
    for b, v in enumerate(vals):
        if not 1 <= v <= int(Fr):
            raise ValueError(f"n_frames[{b}] = {v} is outside 1..Fr={int(Fr)}")
    return vals


def check_n_samples(n_samples, B, T, rule=None):
    """The per-row sample counts of a ragged batch of audio (B, T) as a list of B Python ints, 1 <= n <= T; anything else
    raises ValueError (a host check: nothing is launched).  Accepted: what `check_n_frames` accepts.  `rule`: an analyser's
    row-length rule (`hubert_rule`, `hubert_base_rule`, `crepe_rule`, `f0_ac_rule`, `volume_rule`, `slicer_rule`), count -> None or why such a row is too short."""
    vals = _check_counts("n_samples", n_samples, B)
    for b, v in enumerate(vals):
        if not 1 <= v <= int(T):
            raise ValueError(f"n_samples[{b}] = {v} is outside 1..T={int(T)}")
    for b, v in enumerate(vals if rule is not None else ()):
        reason = rule(v)
        if reason is not None:
            raise ValueError(f"n_samples[{b}] = {v} {reason}")
    return vals


def hubert_rule(n):
    """The units encoder's row-length rule: a row must be long enough for the conv stack (`hubert_frames(n) >= 1`)."""
    return None if hubert_frames(n) >= 1 else "samples are too short for the conv stack"


def hubert_base_rule(n):
    """The row-length rule of the base-form units encoder, which does not pad its input (`hubert_base_frames(n) >= 1`)."""
    return None if hubert_base_frames(n) >= 1 else "samples are too short for the conv stack"


def crepe_rule(hop=80):
    """The CREPE f0 extractor's row-length rule (counts at 16 kHz): at least 3 CREPE frames, for the reflect-padded filters."""
    def rule(n):
        k = crepe_frames(n, hop)
        return None if k >= 3 else f"samples at 16 kHz give {k} CREPE frames; the reflect-padded filters need at least 3"
    return rule


def f0_ac_rule(sr, hop, f0_min):
    """The autocorrelation f0 extractor's row-length rule: a row must hold one analysis window of 3 / f0_min seconds."""
    def rule(n):
        return None if f0_ac_frames(n, sr, hop, f0_min) >= 1 else \
            f"samples at {sr} Hz are shorter than one analysis window of 3 / f0_min = {3.0 / f0_min:.4f} s"
    return rule


def volume_rule(hop):
    """The volume's row-length rule: a row must be longer than its reflect padding, n > (hop + 1) // 2."""
    pad = (int(hop) + 1) // 2
    return lambda n: None if n > pad else f"samples are not longer than the reflect padding {pad}"


def slicer_rule(n):
    """The silence slicer's row-length rule: a row needs at least 1 sample (every such row has a frame)."""
    return None if n >= 1 else "samples: the slicer needs at least 1"


def check_loss_scales(n_samples, n_ffts):
    """The spectral loss over rows of different length (`n_samples`: the list `check_n_samples` returned): at every scale
    some row must hold a whole frame (n_samples[b] >= n_fft), else there is nothing to average (ValueError, a host check)."""
    for n in n_ffts:
        if max(n_samples) < int(n):
            raise ValueError(f"n_samples: no row holds a whole frame at scale n_fft = {int(n)} (longest row: {max(n_samples)} "
                             "samples)")


def loss_norms(n_samples, n_ffts, hops=None):
    """The spectral loss's two denominators per scale over rows of `n_samples` samples: [(cells, rows_ne)], cells = sum_b F_b *
    (n_fft // 2 + 1) with F_b = (n_b - n_fft) // hop + 1 frames (0 for a row shorter than n_fft), rows_ne the rows with a frame.
    hops: one hop per scale (default: hop = n_fft).  What `ddsp_rss_loss` forms from the local rows, or from the
    rows of the global batch when it is given them."""
    hops = [int(n) for n in n_ffts] if hops is None else [int(h) for h in hops]
    out = []
    for n_fft, hop in zip((int(n) for n in n_ffts), hops):
        frames = [(int(n) - n_fft) // hop + 1 for n in n_samples if int(n) >= n_fft]
        out.append((sum(frames) * (n_fft // 2 + 1), len(frames)))
    return out


def check_global_n_samples(global_n_samples, n_samples):
    """The sample counts of every rank's rows (`RSSLoss.forward(..., global_n_samples=)`) as a list of Python ints: a sequence
    of ints or a CPU integer tensor, every entry positive, the local rows `n_samples` (a checked list) among them (as a
    multiset; a global row may be longer than the local padded length).  ValueError otherwise, a host check."""
    if isinstance(global_n_samples, torch.Tensor):
        n = global_n_samples.numel() if global_n_samples.dim() == 1 else -1
    else:
        try:
            global_n_samples = list(global_n_samples)
        except TypeError:
            raise ValueError("global_n_samples must be a sequence of ints or a CPU integer tensor") from None
        n = len(global_n_samples)
    vals = _check_counts("global_n_samples", global_n_samples, n)
    for b, v in enumerate(vals):
        if v < 1:
            raise ValueError(f"global_n_samples[{b}] = {v} must be positive")
    left = list(vals)
    for b, v in enumerate(n_samples):
        if v not in left:
            raise ValueError(f"n_samples[{b}] = {v} is not among global_n_samples: the global batch holds every rank's rows")
        left.remove(v)
    return vals


# `check_n_samples` with each analyser's rule applied
check_hubert_n_samples = lambda n_samples, B, T: check_n_samples(n_samples, B, T, hubert_rule)                       # noqa: E731
check_hubert_base_n_samples = lambda n_samples, B, T: check_n_samples(n_samples, B, T, hubert_base_rule)             # noqa: E731
check_crepe_n_samples = lambda n_samples, B, T, hop=80: check_n_samples(n_samples, B, T, crepe_rule(hop))           # noqa: E731
check_f0_ac_n_samples = lambda n_samples, B, T, sr, hop, f0_min: check_n_samples(n_samples, B, T, f0_ac_rule(sr, hop, f0_min))  # noqa: E731
check_volume_n_samples = lambda n_samples, B, T, hop: check_n_samples(n_samples, B, T, volume_rule(hop))            # noqa: E731


MAX_MIX = 16                      # speakers in one mix (MixArgs of csrc/u2c.h; the K of a row-mix table)
MAX_RETRIEVE_K = 16               # neighbours of one frame in `Context.units_retrieve_` (RT_KMAX of csrc/retrieve.hip)


def check_mix_rows(ids, w, B, n_spk=None):
    """The per-row speaker-mix tables of `unit2ctrl(..., mix_dev=(ids, w))`: ids (B, K) int32 (1-based) and w (B, K) fp32,
    contiguous tensors on one device, 1 <= K <= 16; anything else raises ValueError (a host check of shapes and dtypes:
    nothing is launched and nothing is read back, so device tables are not inspected).  Tables on the CPU (what a caller builds
    before the upload) are also checked for ids in [1, n_spk] when `n_spk` is given.  -> K."""
    if not (isinstance(ids, torch.Tensor) and isinstance(w, torch.Tensor)):
        raise ValueError("a row mix is a pair of tensors (ids (B, K) int32, w (B, K) fp32)")
    if ids.dtype != torch.int32 or w.dtype != torch.float32:
        raise ValueError(f"a row mix holds int32 ids and fp32 weights, got {ids.dtype} and {w.dtype}")
    if ids.dim() != 2 or tuple(w.shape) != tuple(ids.shape) or ids.shape[0] != int(B):
        raise ValueError(f"a row mix holds two (B={int(B)}, K) tables, got {tuple(ids.shape)} and {tuple(w.shape)}")
    K = int(ids.shape[1])
    if not 1 <= K <= MAX_MIX:
        raise ValueError(f"a row mix holds 1 to {MAX_MIX} speakers per row, got K = {K}")
    if ids.device != w.device:
        raise ValueError("the two tables of a row mix must live on one device")
    if not (ids.is_contiguous() and w.is_contiguous()):
        raise ValueError("the two tables of a row mix must be contiguous")
    if n_spk is not None and not ids.is_cuda and ids.numel() and not (int(ids.min()) >= 1 and int(ids.max()) <= int(n_spk)):
        raise ValueError(f"a row mix holds speaker ids in [1, {int(n_spk)}]")
    return K


def check_mix_frames(ids, w, B, Fr):
    """The per-frame speaker-mix tables of `unit2ctrl_framemix`: ids (B, K) int32 (1-based) and w (B, Fr, K) fp32, contiguous
    tensors on one device, 1 <= K <= 16; anything else raises ValueError (a host check of shapes and dtypes, as
    `check_mix_rows`: nothing is launched or read back; the ids of device tables are the kernel's to check).  -> K."""
    if not (isinstance(ids, torch.Tensor) and isinstance(w, torch.Tensor)):
        raise ValueError("a frame mix is a pair of tensors (ids (B, K) int32, w (B, Fr, K) fp32)")
    if ids.dtype != torch.int32 or w.dtype != torch.float32:
        raise ValueError(f"a frame mix holds int32 ids and fp32 weights, got {ids.dtype} and {w.dtype}")
    if ids.dim() != 2 or ids.shape[0] != int(B) or tuple(w.shape) != (int(B), int(Fr), ids.shape[1]):
        raise ValueError(f"a frame mix holds ids (B={int(B)}, K) and weights (B={int(B)}, Fr={int(Fr)}, K), got "
                         f"{tuple(ids.shape)} and {tuple(w.shape)}")
    K = int(ids.shape[1])
    if not 1 <= K <= MAX_MIX:
        raise ValueError(f"a frame mix holds 1 to {MAX_MIX} speakers per frame, got K = {K}")
    if ids.device != w.device:
        raise ValueError("the two tables of a frame mix must live on one device")
    if not (ids.is_contiguous() and w.is_contiguous()):
        raise ValueError("the two tables of a frame mix must be contiguous")
    return K


def mix_rows(mixes, K, n_spk=None):
    """[{speaker id: weight} | int id, ...] -> CPU tables (ids (B, K) int32, w (B, K) fp32) in each dict's own order, short rows
    padded with {id 1, weight 0}; a plain id is the row {id: 1.0}.  ValueError for a row with no or more than K speakers, or an
    id outside [1, n_spk]."""
    ids = torch.ones(len(mixes), int(K), dtype=torch.int32)
    w = torch.zeros(len(mixes), int(K), dtype=torch.float32)
    for b, mix in enumerate(mixes):
        if not isinstance(mix, dict):
            mix = {int(mix): 1.0}
        if not 1 <= len(mix) <= int(K):
            raise ValueError(f"row {b}: a speaker mix holds 1 to {int(K)} ids, got {len(mix)}")
        for k, (i, v) in enumerate(mix.items()):
            if int(i) < 1 or (n_spk is not None and int(i) > int(n_spk)):
                raise ValueError(f"row {b}: speaker id {i} is outside [1, {n_spk}]")
            ids[b, k], w[b, k] = int(i), float(v)
    return ids, w


def formant_factor(semitones, bound=24.0):
    """A formant shift in semitones -> its factor, 2 ** (float(s) / 12) as a Python float (the rule of a key: stored to fp32
    where it is used).  ValueError for anything but a finite number with |s| <= bound."""
    if isinstance(semitones, bool) or not isinstance(semitones, (int, float)) or not _math.isfinite(semitones) or \
            abs(semitones) > bound:
        raise ValueError(f"formant must be a finite number of semitones with |formant| <= {bound:g}, got {semitones!r}")
    return 2 ** (float(semitones) / 12)


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libddsp_amd needs device tensors (no CPU fallback)")
    if not t.is_contiguous():
        raise ValueError("libddsp_amd needs contiguous tensors")
    return t.data_ptr()


class Context:
    """One `ddsp_ctx` (scratch arena + constant tables) bound to a device; use one per stream/thread."""

    def __init__(self, device):
        self.lib = load_library()
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("libddsp_amd runs on a HIP device only (no CPU fallback); got device=%r" % (device,))
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: libddsp_amd cannot run (no CPU fallback)")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        h = _vp()
        rc = self.lib.ddsp_ctx_create(ctypes.byref(h), self.device.index)
        if rc != DDSP_OK:
            raise RuntimeError(f"ddsp_ctx_create failed with {rc}")
        self.handle = h

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.ddsp_ctx_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # -- helpers ------------------------------------------------------------------------------
    def _stream(self):
        """The torch stream current on this thread.  A context's scratch arena and lazily built tables are ordered by ONE
        stream (include/ddsp_amd.h: one context per stream); when a caller switches streams under a cached context
        (`with torch.cuda.stream(s):`), the new stream first waits for everything the context queued on the old one, so a
        half-built table or a scratch region still being read is never touched.  Concurrency across streams
        needs a context per stream (`Context(device)` + `use_context`)."""
        s = torch.cuda.current_stream(self.device)
        last = getattr(self, "_last_stream", None)
        if last is not None and last != s and not torch.cuda.is_current_stream_capturing():
            s.wait_stream(last)
        self._last_stream = s
        return s.cuda_stream

    def _check(self, rc, what):
        if rc == DDSP_OK:
            return
        msg = self.lib.ddsp_last_error(self.handle)
        msg = msg.decode() if msg else ""
        if rc == DDSP_ERR_ARG:
            raise ValueError(f"{what}: {msg}")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")

    def call(self, name, *args):
        if getattr(self, "_frozen", False):
            raise RuntimeError("this ddsp context belongs to a captured HIP graph (its scratch arena and tables are "
                               "referenced by the graph's kernels); use another context for eager calls")
        rc = getattr(self.lib, name)(self.handle, self._stream(), *args)
        self._check(rc, name)

    def freeze(self):
        """After a HIP graph has captured calls made through this context: refuse every further eager call, so that
        nothing can regrow or overwrite the scratch memory the captured kernels point into."""
        self._frozen = True

    def poll_error(self):
        """Raises ValueError if a kernel of an earlier call met a device-side contract violation (a speaker id outside
        the table); synchronise the stream first to be sure the call has run."""
        self._check(self.lib.ddsp_ctx_poll_error(self.handle), "ddsp_ctx_poll_error")

    # -- product arithmetic of the inference contractions ---------------------------------------
    @property
    def math(self):
        return self.lib.ddsp_ctx_get_math(self.handle)

    @property
    def fir_math(self):
        """The `math` argument the model forwards pass to `ddsp_ltv_fir` for this context's mode."""
        return FIR_FP32 if self.math == MATH_FP32 else FIR_SPLIT_BF16

    def set_math(self, math):
        """MATH_SPLIT_BF16 (default) or MATH_FP32: `ddsp_ctx_set_math`; the model forwards pass the same value to
        `ddsp_ltv_fir`."""
        self._check(self.lib.ddsp_ctx_set_math(self.handle, int(math)), "ddsp_ctx_set_math")

    # -- measurement ---------------------------------------------------------------------------
    def profile_begin(self, families=None):
        """Arms HIP-event timing for the named kernel families (all when None)."""
        mask = 0
        for f in (families if families is not None else FAMILIES):
            mask |= 1 << FAMILIES.index(f)
        self._check(self.lib.ddsp_profile_begin(self.handle, mask), "ddsp_profile_begin")

    def profile_mask(self, families):
        """While armed: bracket only `families` from now on ([] pauses); the records taken so far are kept."""
        mask = 0
        for f in families:
            mask |= 1 << FAMILIES.index(f)
        self._check(self.lib.ddsp_profile_mask(self.handle, mask), "ddsp_profile_mask")

    def profile_end(self):
        """-> {family: {launches, ms_total, flops_total, bytes_total}} (waits for the recorded events)."""
        buf = (ProfEntry * 32)()
        n = _int(0)
        self._check(self.lib.ddsp_profile_end(self.handle, buf, 32, ctypes.byref(n)), "ddsp_profile_end")
        return {buf[i].name.decode(): {"launches": buf[i].launches, "ms_total": buf[i].ms_total,
                                       "flops_total": buf[i].flops_total, "bytes_total": buf[i].bytes_total}
                for i in range(n.value)}

    # -- a1 ------------------------------------------------------------------------------------
    def upsample(self, x, hop):
        B, Fr, C = x.shape
        x = x.contiguous().float()
        out = torch.empty(B, Fr * hop, C, device=x.device, dtype=torch.float32)
        self.call("ddsp_upsample", _ptr(x), B, Fr, C, int(hop), _ptr(out))
        return out

    # -- a1-a3 ---------------------------------------------------------------------------------
    def phase_scan(self, f0_frames, hop, sr, initial_phase=None, precise=True, comb_mode=COMB_NONE,
                   want_rot=False, want_phase=False, want_f0=False):
        f0 = f0_frames.reshape(f0_frames.shape[0], -1).contiguous().float()
        B, Fr = f0.shape
        T = Fr * hop
        dev = f0.device
        mk = lambda: torch.empty(B, T, device=dev, dtype=torch.float32)
        rot = mk() if want_rot else None
        phase = mk() if want_phase else None
        comb = mk() if comb_mode != COMB_NONE else None
        f0_up = mk() if want_f0 else None
        pf = torch.empty(B, Fr, device=dev, dtype=torch.float32)
        ip = None if initial_phase is None else initial_phase.reshape(-1).contiguous().float()
        self.call("ddsp_phase_scan", _ptr(f0), _ptr(ip), B, Fr, int(hop), int(sr), 1 if precise else 0,
                  int(comb_mode), _ptr(rot), _ptr(phase), _ptr(comb), _ptr(f0_up), _ptr(pf))
        return {"rot": rot, "phase": phase, "comb": comb, "f0_up": f0_up, "phase_frames": pf}

    # -- a4 ------------------------------------------------------------------------------------
    def unit2ctrl(self, weights, units, f0_frames, phase_frames, volume, spk_id, spk_mix_dict, n_out, n_frames=None,
                  mix_dev=None):
        """n_frames: the (B,) int32 device tensor of a ragged batch (`ragged_counts`); units past a row's count must be 0.
        mix_dev: (ids (B, K) int32, w (B, K) fp32) device tables, a speaker mix per row (`check_mix_rows`) in place of
        `spk_id` / `spk_mix_dict`; the kernels read them when they run (a captured graph follows edits)."""
        B, Fr, _ = units.shape
        if mix_dev is not None:
            if spk_mix_dict is not None:
                raise ValueError("unit2ctrl: mix_dev= and spk_mix_dict are mutually exclusive")
            ids, w = mix_dev
            K = check_mix_rows(ids, w, B, weights.n_spk)
            if not ids.is_cuda or ids.device != units.device:
                raise ValueError("unit2ctrl: the mix_dev tables must be on the units' device")
            ctrl = torch.empty(B, Fr, n_out, device=units.device, dtype=torch.float32)
            frames = [units.contiguous().float()] + [t.reshape(B, Fr).contiguous().float() for t in (f0_frames, phase_frames, volume)]
            args = [_ptr(t) for t in frames] + [_ptr(ids), _ptr(w), K, B, Fr]
            self.call("ddsp_unit2ctrl_fwd_rowmix", ctypes.byref(weights), *args, _ptr(n_frames), _ptr(ctrl))
            return ctrl
        ctrl = torch.empty(B, Fr, n_out, device=units.device, dtype=torch.float32)
        hold, args = self._u2c_inputs(units, f0_frames, phase_frames, volume, spk_id, spk_mix_dict)
        self.call("ddsp_unit2ctrl_fwd", ctypes.byref(weights), *args, _ptr(n_frames), _ptr(ctrl))
        return ctrl

    def unit2ctrl_framemix(self, weights, units, f0_frames, phase_frames, volume, ids, w, n_out, n_frames=None):
        """`unit2ctrl(mix_dev=)` with the weights of every FRAME: ids (B, K) int32 and w (B, Fr, K) fp32 device tables
        (`check_mix_frames`); frame i of row b adds sum_k w[b, i, k] * spk_embed[ids[b, k] - 1] in slot order.  n_frames as
        `unit2ctrl` takes it.  The kernels read the tables when they run (a captured graph follows edits); an id outside
        [1, n_spk] sets the device error word."""
        B, Fr, _ = units.shape
        K = check_mix_frames(ids, w, B, Fr)
        if not ids.is_cuda or ids.device != units.device:
            raise ValueError("unit2ctrl_framemix: the mix tables must be on the units' device")
        ctrl = torch.empty(B, Fr, n_out, device=units.device, dtype=torch.float32)
        frames = [units.contiguous().float()] + [t.reshape(B, Fr).contiguous().float() for t in (f0_frames, phase_frames, volume)]
        args = [_ptr(t) for t in frames] + [_ptr(ids), _ptr(w), K, B, Fr]
        self.call("ddsp_unit2ctrl_fwd_framemix", ctypes.byref(weights), *args, _ptr(n_frames), _ptr(ctrl))
        return ctrl

    def mix_timeline(self, table_dev, bp_off, bp_frame, bp_w, job_ids, N_max):
        """One launch (`ddsp_mix_timeline`): the speaker timelines of J jobs -> the per-frame mix tables of a render group.
        table_dev (R, 6) int32 device rows of `infer_offline.job_table`; bp_off (J + 1,) int32, bp_frame (P,) int32 (file
        frames), bp_w (P, K) fp32, job_ids (J, K) int32, all contiguous on the device -> (ids (R, K) int32, w (R, N_max, K)
        fp32): the piecewise-linear interpolation of each row's job at its file frames, exact zeros past a row's count, and a
        padding row (ids 1, weights 0) for a job outside [0, J).  Nothing is read back."""
        def table(name, t, dtype, dim):
            if not (isinstance(t, torch.Tensor) and t.device == self.device and t.dtype == dtype and t.dim() == dim
                    and t.is_contiguous()):
                raise ValueError(f"mix_timeline: {name} must be a contiguous {dim}-d {dtype} tensor on {self.device}")
            return t
        table("the table", table_dev, torch.int32, 2)
        table("bp_off", bp_off, torch.int32, 1)
        table("bp_frame", bp_frame, torch.int32, 1)
        table("bp_w", bp_w, torch.float32, 2)
        table("job_ids", job_ids, torch.int32, 2)
        R, J, P, K = table_dev.shape[0], job_ids.shape[0], bp_frame.numel(), job_ids.shape[1]
        if table_dev.shape[1] != 6 or bp_off.numel() != J + 1 or tuple(bp_w.shape) != (P, K) or J < 1 or P < 1 or \
                not 1 <= K <= MAX_MIX or int(N_max) < 1:
            raise ValueError(f"mix_timeline: a table (R, 6), bp_off (J + 1,), bp_frame (P,), bp_w (P, K) and job_ids (J, K) with "
                             f"J, P, N_max >= 1 and 1 <= K <= {MAX_MIX}; got {tuple(table_dev.shape)}, {tuple(bp_off.shape)}, "
                             f"{tuple(bp_frame.shape)}, {tuple(bp_w.shape)}, {tuple(job_ids.shape)}, N_max = {N_max}")
        ids = torch.empty(R, K, device=self.device, dtype=torch.int32)
        w = torch.empty(R, int(N_max), K, device=self.device, dtype=torch.float32)
        if R:
            self.call("ddsp_mix_timeline", _ptr(table_dev), R, J, _ptr(bp_off), _ptr(bp_frame), _ptr(bp_w), P, _ptr(job_ids), K,
                      int(N_max), _ptr(ids), _ptr(w))
        return ids, w

    # -- ragged batches (include/ddsp_amd.h): held frames, cropped signals, the noise draw ---------
    def ragged_counts(self, counts):
        """counts: the list `check_n_frames` returned -> the (B,) int32 device tensor the ragged calls take (one upload)."""
        return torch.tensor(counts, dtype=torch.int32).to(self.device)

    @staticmethod
    def _counts_dev(t, B):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.numel() == B and t.is_contiguous()):
            raise ValueError("counts_dev must be a contiguous (B,) int32 device tensor (`ragged_counts`)")
        return t

    def ragged_frames(self, x, n_dev, hold, out=None):
        """x (B,Fr,C) or (B,Fr) -> frames past a row's count replaced by its last frame (hold) or by 0; `out=x`: in place."""
        B, Fr = x.shape[0], x.shape[1]
        C = x.numel() // max(B * Fr, 1)
        if out is None:
            x = x.contiguous().float()
            out = torch.empty_like(x)
        elif x.dtype != torch.float32 or not x.is_contiguous() or out.data_ptr() != x.data_ptr():
            raise ValueError("ragged_frames: `out` is for the in-place call, out=x, on a contiguous fp32 tensor")
        self.call("ddsp_ragged_frames", _ptr(x), _ptr(n_dev), B, Fr, C, 1 if hold else 0, _ptr(out))
        return out

    def ragged_frames_adjoint_(self, d, n_dev):
        """In place on a gradient d (B,Fr,C) fp32: the adjoint of `ragged_frames(hold=True)` - frame n_b - 1 of every row
        collects the gradient of the frames behind it (ascending order), which are then 0."""
        if d.dtype != torch.float32 or not d.is_contiguous() or d.dim() not in (2, 3):
            raise ValueError("ragged_frames_adjoint_: a contiguous fp32 (B, Fr, C) or (B, Fr) tensor")
        B, Fr = d.shape[0], d.shape[1]
        self.call("ddsp_ragged_frames_adjoint", _ptr(d), _ptr(self._counts_dev(n_dev, B)), B, Fr, d.numel() // max(B * Fr, 1))
        return d

    def ragged_crop_(self, n_dev, Fr, hop, *signals):
        """In place: up to three (B, Fr*hop) fp32 signals are set to 0 from sample n_b * hop on."""
        xs = [s for s in signals if s is not None]
        for s in xs:
            if s.dtype != torch.float32 or not s.is_contiguous() or s.dim() != 2 or s.shape[1] != int(Fr) * int(hop):
                raise ValueError("ragged_crop_: contiguous fp32 (B, Fr*hop) signals")
        for i in range(0, len(xs), 3):
            grp = xs[i:i + 3] + [None] * (3 - len(xs[i:i + 3]))
            self.call("ddsp_ragged_crop", _ptr(grp[0]), _ptr(grp[1]), _ptr(grp[2]), _ptr(n_dev), grp[0].shape[0], int(Fr), int(hop))

    def ragged_noise(self, noise, noise_seed, n_dev, B, Fr, hop):
        """The unit-noise draw (B, Fr*hop) of a ragged batch for EXC_UNIT_NOISE: the caller's `noise` or a hash of the seed
        inside a row, 0.5 (-> exactly 0 excitation) past its end."""
        out = torch.empty(B, Fr * hop, device=self.device, dtype=torch.float32)
        if noise is not None:
            noise = noise.contiguous().float()
            if tuple(noise.shape) != (B, Fr * hop):
                raise ValueError(f"noise must be (B, Fr*hop) = {(B, Fr * hop)}, got {tuple(noise.shape)}")
        self.call("ddsp_ragged_noise", _ptr(noise), int(noise_seed) & ((1 << 64) - 1), _ptr(n_dev), B, Fr, int(hop), _ptr(out))
        return out

    def dataset_gather(self, view, B, Fr_out, triples=None, perm=None, cursor=0, seed=0, len_rows=None, crop_frames=0,
                       waveform_sec=0.0, out=None):
        """One training batch of B rows from a packed dataset (`DatasetView`; `data_loaders.AudioDataset` builds one) in one
        launch.  triples (B,3) int32 device: the rows' (file, start_frame, unit_idx), injected; or perm (n,) int32 device
        with `cursor` and `seed`: drawn in the kernel.  len_rows (B,) int32 device: the rows' own frame counts (injected only),
        else `crop_frames` for every row; frames past a row's count are exact zeros.  `out`: a dict of preallocated contiguous
        outputs to write into.  -> {audio (B,Fr_out*hop), units (B,Fr_out,C), f0 (B,Fr_out,1), volume (B,Fr_out) fp32, spk_id
        (B,1) int64, draws (B,3) int32: the triples used}.  A triple outside its file raises ValueError from the NEXT call
        (or `poll_error()` after a synchronise): the kernel cannot fail the call that launched it."""
        B, Fr_out = int(B), int(Fr_out)
        for name, t, shape in (("triples", triples, (B, 3)), ("perm", perm, None), ("len_rows", len_rows, (B,))):
            if t is not None and (t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous()
                                  or (shape is not None and tuple(t.shape) != shape) or (shape is None and t.dim() != 1)):
                raise ValueError(f"dataset_gather: {name} must be a contiguous int32 device tensor"
                                 + (f" of shape {shape}" if shape else " of one dimension"))
        shapes = {"audio": ((B, Fr_out * view.hop), torch.float32), "units": ((B, Fr_out, view.n_unit), torch.float32),
                  "f0": ((B, Fr_out, 1), torch.float32), "volume": ((B, Fr_out), torch.float32),
                  "spk_id": ((B, 1), torch.int64), "draws": ((B, 3), torch.int32)}
        if out is None:
            out = {k: torch.empty(shape, device=self.device, dtype=dt) for k, (shape, dt) in shapes.items()}
        else:
            for k, (shape, dt) in shapes.items():
                if tuple(out[k].shape) != shape or out[k].dtype != dt:
                    raise ValueError(f"dataset_gather: out[{k!r}] must be {dt} of shape {shape}")
        self.call("ddsp_dataset_gather", ctypes.byref(view), _ptr(triples), _ptr(perm), 0 if perm is None else perm.shape[0],
                  int(cursor), int(seed) & ((1 << 64) - 1), _ptr(len_rows), int(crop_frames), float(waveform_sec), B, Fr_out,
                  *[_ptr(out[k]) for k in ("audio", "units", "f0", "volume", "spk_id", "draws")])
        return {k: out[k] for k in shapes}

    def unit2ctrl_bwd(self, weights, grads, units, f0_frames, phase_frames, volume, spk_id, spk_mix_dict, n_out,
                      d_ctrl, want_ctrl=False, n_frames=None):
        """Back-propagates d_ctrl (B,Fr,n_out) into the tensors `grads` points at (same struct layout as `weights`).
        n_frames: the (B,) int32 device tensor of a ragged batch (`ragged_counts`); units and d_ctrl past a row's count must
        be 0 and the other inputs finite there."""
        B, Fr, _ = units.shape
        d_ctrl = d_ctrl.contiguous().float()
        ctrl = torch.empty(B, Fr, n_out, device=units.device, dtype=torch.float32) if want_ctrl else None
        hold, args = self._u2c_inputs(units, f0_frames, phase_frames, volume, spk_id, spk_mix_dict)
        n_dev = None if n_frames is None else self._counts_dev(n_frames, B)
        self.call("ddsp_unit2ctrl_bwd", ctypes.byref(weights), *args, _ptr(n_dev), _ptr(d_ctrl), ctypes.byref(grads), _ptr(ctrl))
        return ctrl

    def _u2c_inputs(self, units, f0_frames, phase_frames, volume, spk_id, spk_mix_dict):
        """The inputs every unit2ctrl entry point shares -> (the tensors to hold until the call is queued, its arguments from
        `units` to `Fr`); the speaker is a mix (host arrays) or spk_id (1 or B ids on the device)."""
        B, Fr, _ = units.shape
        dev = units.device
        units = units.contiguous().float()
        f0 = f0_frames.reshape(B, Fr).contiguous().float()
        ph = phase_frames.reshape(B, Fr).contiguous().float()
        vol = volume.reshape(B, Fr).contiguous().float()
        if spk_mix_dict is not None:
            n_mix = len(spk_mix_dict)
            ids = (_i64 * max(n_mix, 1))(*[int(k) for k in spk_mix_dict.keys()])
            ws = (_f32 * max(n_mix, 1))(*[float(v) for v in spk_mix_dict.values()])
            sid, n_sid = None, 0
        else:
            n_mix, ids, ws = 0, None, None
            sid = spk_id.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
            n_sid = sid.numel()
            if n_sid not in (1, B):
                raise ValueError(f"spk_id must hold 1 or B={B} ids, got {n_sid}")
        return (units, f0, ph, vol, sid), (_ptr(units), _ptr(f0), _ptr(ph), _ptr(vol), _ptr(sid), n_sid, ids, ws, n_mix, B, Fr)

    def unit2ctrl_keep(self, weights, units, f0_frames, phase_frames, volume, spk_id, spk_mix_dict, n_out, n_frames=None):
        """Training forward (fp32 products) that keeps its activations: -> (ctrl (B,Fr,n_out), keep) where `keep` is the
        uint8 device tensor `unit2ctrl_bwd_kept` back-propagates from (the caller holds it until then).
        n_frames: the (B,) int32 device tensor of a ragged batch, as `unit2ctrl` takes it."""
        B, Fr, _ = units.shape
        nbytes = int(self.lib.ddsp_unit2ctrl_keep_bytes(ctypes.byref(weights), B, Fr))
        if nbytes < 0:
            raise ValueError("ddsp_unit2ctrl_keep_bytes: bad shape")
        keep = torch.empty(nbytes, device=units.device, dtype=torch.uint8)
        ctrl = torch.empty(B, Fr, n_out, device=units.device, dtype=torch.float32)
        hold, args = self._u2c_inputs(units, f0_frames, phase_frames, volume, spk_id, spk_mix_dict)
        n_dev = None if n_frames is None else self._counts_dev(n_frames, B)
        self.call("ddsp_unit2ctrl_fwd_keep", ctypes.byref(weights), *args, _ptr(n_dev), _ptr(keep), nbytes, _ptr(ctrl))
        return ctrl, keep

    def unit2ctrl_bwd_kept(self, weights, grads, units, f0_frames, phase_frames, volume, spk_id, spk_mix_dict, keep, d_ctrl,
                           n_frames=None):
        """Back-propagates d_ctrl from the activations `unit2ctrl_keep` left in `keep` (no second forward); `n_frames` as
        that call had it (`unit2ctrl_bwd` says what a ragged batch asks of the inputs)."""
        d_ctrl = d_ctrl.contiguous().float()
        hold, args = self._u2c_inputs(units, f0_frames, phase_frames, volume, spk_id, spk_mix_dict)
        n_dev = None if n_frames is None else self._counts_dev(n_frames, units.shape[0])
        self.call("ddsp_unit2ctrl_bwd_kept", ctypes.byref(weights), *args, _ptr(n_dev), _ptr(keep), keep.numel(), _ptr(d_ctrl),
                  ctypes.byref(grads))

    # -- a5-a6 ---------------------------------------------------------------------------------
    def fir_from_ctrl(self, mode, ctrl2d, col0, n_mag, rows, sr, f0_frames=None):
        """ctrl2d :: (rows, ld) contiguous; the filter's control values are columns [col0, col0+n_mag)."""
        ld = ctrl2d.shape[-1]
        n = 2 * (n_mag - 1)
        ir = torch.empty(rows, n, device=ctrl2d.device, dtype=torch.float32)
        base = _ptr(ctrl2d) + 4 * col0
        f0 = None if f0_frames is None else f0_frames.reshape(-1).contiguous().float()
        self.call("ddsp_fir_from_ctrl", int(mode), base, ld, int(n_mag), _ptr(f0), rows, int(sr), _ptr(ir))
        return ir

    def fir_from_ctrl_group(self, ctrl2d, problems, rows, sr, f0_frames=None):
        """`problems`: up to three (mode, col0, n_mag) of one control matrix -> their filters, the bits of `fir_from_ctrl`
        each; at large inference batches in two launches (`ddsp_fir_from_ctrl_group`).  f0_frames: for the DYNAMIC ones."""
        f0 = None if f0_frames is None else f0_frames.reshape(-1).contiguous().float()
        irs = [torch.empty(rows, 2 * (n_mag - 1), device=ctrl2d.device, dtype=torch.float32) for _, _, n_mag in problems]
        table = (FirProblem * len(problems))(*[
            FirProblem(int(mode), int(col0), int(n_mag), _ptr(f0) if mode == FIR_DYNAMIC else None, _ptr(ir))
            for (mode, col0, n_mag), ir in zip(problems, irs)])
        self.call("ddsp_fir_from_ctrl_group", _ptr(ctrl2d), ctrl2d.shape[-1], rows, int(sr), table, len(problems))
        return irs

    # -- a7 ------------------------------------------------------------------------------------
    def ltv_fir(self, audio, ir, B, Fr, hop, excitation=EXC_AUDIO, noise_seed=0, add_in=None, want_out=True,
                math=FIR_FP32):
        """Returns (filtered | None, filtered + add_in | None).  math: FIR_FP32 or FIR_SPLIT_BF16 (inference)."""
        n = ir.shape[-1]
        # the kernel reads B * Fr * hop samples and B * Fr filters whatever the tensors hold: sizes are checked here
        for name, t, want in (("audio", audio, B * Fr * hop), ("add_in", add_in, B * Fr * hop), ("ir", ir, B * Fr * n)):
            if t is not None and t.numel() != want:
                raise ValueError(f"ltv_fir: {name} holds {t.numel()} values, B * Fr * {'n' if name == 'ir' else 'hop'} = {want} "
                                 f"expected (B = {B}, Fr = {Fr}, hop = {hop})")
        mk = lambda: torch.empty(B, Fr * hop, device=ir.device, dtype=torch.float32)
        out = mk() if want_out else None
        out_sum = mk() if add_in is not None else None
        self.call("ddsp_ltv_fir", _ptr(audio), int(excitation), int(noise_seed), _ptr(ir), B, Fr, int(hop), int(n),
                  _ptr(add_in), _ptr(out), _ptr(out_sum), int(math))
        return out, out_sum


    # -- backward of a5-a8 ---------------------------------------------------------------------
    def ltv_fir_bwd(self, audio, ir, d_out, B, Fr, hop, excitation=EXC_AUDIO, noise_seed=0, want_d_audio=True,
                    want_d_ir=True):
        n = ir.shape[-1]
        for name, t, want in (("audio", audio, B * Fr * hop), ("d_out", d_out, B * Fr * hop), ("ir", ir, B * Fr * n)):
            if t is not None and t.numel() != want:
                raise ValueError(f"ltv_fir_bwd: {name} holds {t.numel()} values, B * Fr * {'n' if name == 'ir' else 'hop'} = {want} "
                                 f"expected (B = {B}, Fr = {Fr}, hop = {hop})")
        d_out = d_out.contiguous().float()
        d_audio = torch.empty(B, Fr * hop, device=ir.device, dtype=torch.float32) if want_d_audio else None
        d_ir = torch.empty(B * Fr, n, device=ir.device, dtype=torch.float32) if want_d_ir else None
        self.call("ddsp_ltv_fir_bwd", _ptr(audio), int(excitation), int(noise_seed), _ptr(ir), _ptr(d_out), B, Fr,
                  int(hop), int(n), _ptr(d_audio), _ptr(d_ir))
        return d_audio, d_ir

    def fir_from_ctrl_bwd(self, mode, ctrl2d, col0, n_mag, rows, sr, d_ir, d_ctrl2d, f0_frames=None):
        """Writes d ctrl into columns [col0, col0+n_mag) of d_ctrl2d (rows, ld); d_ir is consumed (scaled in place)."""
        f0 = None if f0_frames is None else f0_frames.reshape(-1).contiguous().float()
        self.call("ddsp_fir_from_ctrl_bwd", int(mode), _ptr(ctrl2d) + 4 * col0, ctrl2d.shape[-1], int(n_mag), _ptr(f0),
                  rows, int(sr), _ptr(d_ir), _ptr(d_ctrl2d) + 4 * col0, d_ctrl2d.shape[-1])

    # -- front-end steps -----------------------------------------------------
    def volume_extract(self, audio, hop, n_samples=None):
        """audio (B,T) fp32 -> (B, int(T // hop) + 1) block RMS with numpy-'reflect' padding (ddsp/vocoder.py:116-137).
        `hop` may be a non-integral float (an input at another rate than the model's: block_size * sr / model_sr); an
        integral one, int or float, takes the integer entry point.
        `n_samples` (a sequence of B ints or a CPU integer tensor (B,), integral hop only): a RAGGED batch - row b reflects at
        its own ends, carries n_samples[b] // hop + 1 frames and is 0 after them; its padding is never read."""
        audio = audio.contiguous().float()
        B, T = audio.shape
        if n_samples is not None and not float(hop).is_integer():
            raise ValueError("volume_extract: a ragged batch needs an integral hop")
        vals = None if n_samples is None else check_volume_n_samples(n_samples, B, T, hop)
        if not float(hop).is_integer():
            hop = float(hop)
            out = torch.empty(B, int(T // hop) + 1, device=audio.device, dtype=torch.float32)
            self.call("ddsp_volume_extract_frac", _ptr(audio), B, T, hop, _ptr(out))
            return out
        out = torch.empty(B, T // int(hop) + 1, device=audio.device, dtype=torch.float32)
        if B:
            n_dev = None if vals is None else self.ragged_counts(vals)
            self.call("ddsp_volume_extract", _ptr(audio), B, T, _ptr(n_dev), int(hop), _ptr(out))
        return out

    def align_units(self, units, n_frames, ratio, n_units_dev=None, n_out_dev=None):
        """units (B,Lu,C) -> (B,n_frames,C), row i = units[:, min(rint(fp32(ratio)*i), Lu-1)] (ddsp/vocoder.py:201-211).
        `n_units_dev`, `n_out_dev` (both or neither; (B,) int32 device tensors, `ragged_counts`): a RAGGED batch - row b gathers
        its own n_out[b] frames from its own n_units[b] unit rows and is 0 after them."""
        if (n_units_dev is None) != (n_out_dev is None):
            raise ValueError("align_units: a ragged batch needs both n_units_dev and n_out_dev")
        units = units.contiguous().float()
        B, Lu, C = units.shape
        out = torch.empty(B, int(n_frames), C, device=units.device, dtype=torch.float32)
        if B == 0 or int(n_frames) == 0:
            return out
        self.call("ddsp_align_units", _ptr(units), B, Lu, C, int(n_frames), float(ratio), _ptr(n_units_dev), _ptr(n_out_dev),
                  _ptr(out))
        return out

    def retime_f0(self, f0, step_num, div, scale, step_dst, n_dst, n_src_dev=None, n_dst_dev=None, keyed=None):
        """f0 (n,) device track -> (n_dst,): numpy.interp(i * step_dst; knots (step_num * j) / div, values fl32(f0 * scale)),
        end values held (enhancer.py:56-62), without leaving the device.
        `n_src_dev`, `n_dst_dev` (both or neither; (B,) int32 device tensors, `ragged_counts`): a RAGGED batch - f0 (B, n_src) ->
        (B, n_dst); row b has n_src_dev[b] knots and n_dst_dev[b] targets of its own, ends held at its own first and last frame,
        0 after its targets.
        `keyed` = (key (B,) int32, div_by_key (n,) fp64, scale_by_key (n,) fp32), device tensors: a ragged batch whose row b
        takes div and scale from entry key[b] of the two tables (`div` and `scale` are then not read; pass None)."""
        if (n_src_dev is None) != (n_dst_dev is None):
            raise ValueError("retime_f0: a ragged batch needs both n_src_dev and n_dst_dev")
        if keyed is not None:
            key, div_tab, scale_tab = keyed
            if n_src_dev is None or div_tab.dtype != torch.float64 or scale_tab.dtype != torch.float32 or \
                    div_tab.numel() != scale_tab.numel() or div_tab.numel() < 1:
                raise ValueError("retime_f0: keyed= needs a ragged batch and tables (n,) fp64 / (n,) fp32")
            f0 = f0.contiguous().float()
            B, n_src = f0.shape
            out = torch.empty(B, int(n_dst), device=f0.device, dtype=torch.float32)
            self.call("ddsp_retime_f0_keyed", _ptr(f0), B, n_src, _ptr(n_src_dev), float(step_num), _ptr(self._counts_dev(key, B)),
                      div_tab.numel(), _ptr(div_tab), _ptr(scale_tab), float(step_dst), int(n_dst), _ptr(n_dst_dev), _ptr(out))
            return out
        solo = n_src_dev is None
        f0 = (f0.reshape(1, -1) if solo else f0).contiguous().float()
        B, n_src = f0.shape
        out = torch.empty(B, int(n_dst), device=f0.device, dtype=torch.float32)
        self.call("ddsp_retime_f0", _ptr(f0), B, n_src, _ptr(n_src_dev), float(step_num), float(div), float(scale), float(step_dst),
                  int(n_dst), _ptr(n_dst_dev), _ptr(out))
        return out[0] if solo else out

    # -- sample-rate conversion ---------------------------------------------
    def resample(self, audio, orig_freq, new_freq, lowpass_filter_width=6, n_dev=None):
        """audio (B,T) or (T,) -> (B, ceil(T*new/orig)): windowed-sinc polyphase (torchaudio.transforms.Resample's algorithm).
        `n_dev` (the (B,) int32 device tensor of the rows' own sample counts, `ragged_counts`): a RAGGED batch (B,T) - what
        follows a row's samples is never read into arithmetic, and its outputs from ceil(n_b * new / orig) on are 0."""
        flat = audio.dim() == 1
        if flat and n_dev is not None:
            raise ValueError("resample: n_dev needs a (B, T) batch")
        x = (audio.reshape(1, -1) if flat else audio).contiguous().float()
        B, T = x.shape
        T_out = self.lib.ddsp_resample_length(T, int(orig_freq), int(new_freq))
        if T_out < 0:
            raise ValueError("resample: bad rates")
        out = torch.empty(B, T_out, device=x.device, dtype=torch.float32)
        if B and T:
            self.call("ddsp_resample", _ptr(x), B, T, _ptr(n_dev), int(orig_freq), int(new_freq), int(lowpass_filter_width), _ptr(out))
        return out[0] if flat else out

    def resample_plan(self, pairs, lowpass_filter_width=6):
        """pairs: up to 13 (orig_freq, new_freq) -> `ResamplePlan`: the tap tables of all of them, built now (the call waits
        for them) and resident together while the plan lives, outside this context's cache of solo tables.  The plan belongs
        to the device: any context of it, a captured one included, may run `resample_keyed` with it."""
        pairs = [(int(a), int(b)) for a, b in pairs]
        if not 1 <= len(pairs) <= 13:
            raise ValueError(f"resample_plan: 1 to 13 rate pairs, got {len(pairs)}")
        n = len(pairs)
        h = _vp()
        self.call("ddsp_resample_keyed_plan", n, (_int * n)(*[a for a, _ in pairs]), (_int * n)(*[b for _, b in pairs]),
                  int(lowpass_filter_width), ctypes.byref(h))
        return ResamplePlan(self.lib, h, pairs, int(lowpass_filter_width), self.device)

    def resample_keyed(self, plan, audio, n_dev, key):
        """audio (B, T) with n_dev[b] samples of its own per row, key (B,) int32 (both device tensors) -> (B, plan.length(T)):
        row b resampled with pair key[b] of the plan - bit for bit `resample` of that row alone at that pair over its own
        outputs (a pair of equal rates copies the row), exactly 0 after them."""
        x = audio.contiguous().float()
        B, T = x.shape
        if plan.device != x.device:
            raise ValueError("resample_keyed: the plan lives on another device")
        out = torch.empty(B, plan.length(T), device=x.device, dtype=torch.float32)
        if B and T:
            self.call("ddsp_resample_keyed", plan.handle, _ptr(x), B, T, _ptr(self._counts_dev(n_dev, B)),
                      _ptr(self._counts_dev(key, B)), _ptr(out))
        return out

    def enhancer_keys(self, f0, cut_frames, max_key, request, thresholds):
        """f0 (S, Fr) -> key (S,) int32 on the device: request[s] >= 0 as it is, -1 the reference's 'auto' rule over the frames
        from `cut_frames` on, decided against `thresholds` (`key_thresholds(max_key)` on the device); clamped to max_key."""
        f0 = f0.contiguous().float()
        S, Fr = f0.shape
        if thresholds.dtype != torch.float32 or thresholds.numel() != int(max_key) + 1:
            raise ValueError("enhancer_keys: thresholds holds max_key + 1 fp32 values")
        key = torch.empty(S, device=f0.device, dtype=torch.int32)
        self.call("ddsp_enhancer_keys", _ptr(f0), S, Fr, int(cut_frames), int(max_key), _ptr(self._counts_dev(request, S)),
                  _ptr(thresholds), _ptr(key))
        return key

    # -- NSF-HiFiGAN post-net building blocks --------------------------------
    # Ragged batches (include/ddsp_amd.h, "Ragged batches of the post-net"): `rows=(B, n_dev, scale)` runs a call over B rows
    # flattened on the time axis, (B * T, C), row b valid for n_dev[b] * scale frames (n_dev: (B,) int32 device tensor of
    # `ragged_counts`, or None for a rectangular batch) and written as 0 after them; rows=None is one utterance, x (T, C): the
    # call and the launches of rows=(1, None, 1).
    @staticmethod
    def _rows(name, rows, T):
        """`rows` of a post-net call over x (T, ...) -> (B, frames per row, n_dev, scale); None is (1, T, None, 1)."""
        B, n_dev, scale = (1, None, 1) if rows is None else rows
        if T % int(B):
            raise ValueError(f"{name}: x must hold B rows of equal padded length")
        return int(B), T // int(B), n_dev, int(scale)

    def conv1d(self, x, w_packed, bias, ktaps, dil, in_slope, residual=None, want_out=True, act_slope=None, w_split=None,
               x_split=False, act_split=False, rows=None):
        """x (T,Cin), w_packed (Cout, ktaps*Cin) -> y (T,Cout) = conv_same(leaky_relu(x, in_slope)) + bias (+ residual).
        Returns y, or (y | None, leaky_relu(y, act_slope)) when act_slope is given (want_out=False skips y itself).
        Split operands (include/ddsp_amd.h, ddsp_conv1d): `w_split` = presplit(w_packed); `x_split`: x is in the split layout;
        `act_split`: write the activated copy in it."""
        T, Cin = x.shape
        Cout = w_packed.shape[0]
        if w_packed.shape[1] != ktaps * Cin:
            raise ValueError("conv1d: packed weight does not match (ktaps, Cin)")
        out = torch.empty(T, Cout, device=x.device, dtype=torch.float32) if want_out else None
        act = torch.empty(T, Cout, device=x.device, dtype=torch.float32) if act_slope is not None else None
        if out is None and act is None:
            raise ValueError("conv1d: nothing to return")
        flags = (CONV_X_SPLIT if x_split else 0) | (CONV_ACT_SPLIT if act_split else 0)
        B, Tr, n_dev, scale = self._rows("conv1d", rows, T)
        self.call("ddsp_conv1d", _ptr(x), _ptr(w_packed), _ptr(bias), B, Tr, Cin, Cout, int(ktaps), int(dil), float(in_slope),
                  _ptr(residual), _ptr(out), _ptr(act), float(act_slope if act_slope is not None else 1.0), _ptr(w_split), flags,
                  _ptr(n_dev), scale)
        return out if act_slope is None else (out, act)

    def gemm_res_ln(self, A_split, W_split, bias, res, gamma, beta, y_split=True, a_fp32=False):
        """X = res + A W^T + bias and Y = LayerNorm(X) * gamma + beta in one launch; W (256, K) pre-split, A (M, K) pre-split or
        (a_fp32) plain fp32 rows."""
        M, K = A_split.shape
        X = torch.empty(M, 256, device=A_split.device, dtype=torch.float32)
        Y = torch.empty(M, 256, device=A_split.device, dtype=torch.float32)
        self.call("ddsp_gemm_res_ln", _ptr(A_split), _ptr(W_split), _ptr(bias), _ptr(res), _ptr(gamma), _ptr(beta), int(M), int(K),
                  _ptr(X), _ptr(Y), (1 if y_split else 0) | (2 if a_fp32 else 0))
        return X, Y

    def u2c_dwconv_pw2(self, glu, taps, dw_bias, W_split, bias, res, gamma, beta, B, n_frames=None, causal=False, fused=True):
        """The conformer's depthwise conv k31 -> SiLU -> pw2 -> residual -> LayerNorm on split-bf16 operands: glu (B*Fr, 512) fp32,
        taps (31, 512), W_split (256, 512) pre-split; n_frames: int32 device tensor of B frame counts or None.  fused: one launch
        (the convolution in the GEMM's operand stage), else the depthwise kernel and then the GEMM.  Returns X, Y (split)."""
        M = glu.shape[0]
        if M % int(B):
            raise ValueError("u2c_dwconv_pw2: glu must hold B utterances of equal padded length")
        X = torch.empty(M, 256, device=glu.device, dtype=torch.float32)
        Y = torch.empty(M, 256, device=glu.device, dtype=torch.float32)
        scratch = None if fused else torch.empty(M, 512, device=glu.device, dtype=torch.float32)
        self.call("ddsp_u2c_dwconv_pw2", _ptr(glu), _ptr(taps), _ptr(dw_bias), _ptr(W_split), _ptr(bias), _ptr(res), _ptr(gamma),
                  _ptr(beta), _ptr(n_frames), int(B), M // int(B), 1 if causal else 0, 1 if fused else 0, _ptr(scratch), _ptr(X), _ptr(Y))
        return X, Y

    def conv1d_pair_supported(self, C, ktaps, dil):
        return bool(self.lib.ddsp_conv1d_pair_supported(self.handle, int(C), int(ktaps), int(dil)))

    def conv1d_pair(self, x, w1, b1, w2, b2, ktaps, dil, slope, want_out=True, want_act=False, rows=None):
        """One ResBlock1 pair of a narrow stage: x (T,C) raw -> (x + c2(leaky_relu(c1_dil(leaky_relu(x)))), its activated copy);
        either may be skipped (None)."""
        T, C = x.shape
        out = torch.empty(T, C, device=x.device, dtype=torch.float32) if want_out else None
        act = torch.empty(T, C, device=x.device, dtype=torch.float32) if want_act else None
        B, Tr, n_dev, scale = self._rows("conv1d_pair", rows, T)
        self.call("ddsp_conv1d_pair", _ptr(x), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), B, Tr, C, int(ktaps), int(dil), float(slope),
                  _ptr(out), _ptr(act), _ptr(n_dev), scale)
        return out, act

    def nsf_source(self, f0, rand_ini, lin_w, lin_b, upp, sr, sine_amp=0.1, n_dev=None):
        """f0 (L,), rand_ini (9,) -> source (L * upp,), or f0 (B, L), rand_ini (B, 9) -> (B, L * upp): one phase scan per row
        from its own initial phases; with n_dev ((B,) int32 device tensor), f0 past a row's count is not read and its source
        is 0 from n_dev[b] * upp on."""
        solo = f0.dim() == 1
        if solo and n_dev is not None:
            raise ValueError("nsf_source: n_dev needs f0 (B, L)")
        if not solo and tuple(rand_ini.shape) != (f0.shape[0], 9):
            raise ValueError(f"nsf_source: rand_ini must be (B, 9) = ({f0.shape[0]}, 9), got {tuple(rand_ini.shape)}")
        L = f0.shape[-1]
        rand_ini = rand_ini.contiguous().float()
        out = torch.empty(*f0.shape[:-1], L * int(upp), device=f0.device, dtype=torch.float32)
        self.call("ddsp_nsf_source", _ptr(f0), _ptr(rand_ini), _ptr(lin_w), _ptr(lin_b), 1 if solo else f0.shape[0], L, int(upp),
                  int(sr), float(sine_amp), _ptr(n_dev), _ptr(out))
        return out

    def nsf_noise_conv(self, src, w, b, K, stride, pad, T_out):
        """src (T_src,) -> (T_out, C), or src (B, T_src) -> (B * T_out, C) with the taps row-local."""
        B, T_src = (1, src.numel()) if src.dim() == 1 else src.shape
        C = w.shape[0]
        out = torch.empty(B * int(T_out), C, device=src.device, dtype=torch.float32)
        self.call("ddsp_nsf_noise_conv", _ptr(src), B, T_src, _ptr(w), _ptr(b), C, int(K), int(stride), int(pad), int(T_out), _ptr(out))
        return out

    def nsf_post(self, x, w, b, K, slope, rows=None):
        """x (T, C) -> (T,), or with `rows` (as in conv1d) x (B * T, C) -> (B, T), 0 past each row's end."""
        C = x.shape[1]
        B, n_dev, scale = (1, None, 1) if rows is None else rows
        T = x.shape[0] // int(B)
        out = torch.empty(int(B), T, device=x.device, dtype=torch.float32)
        self.call("ddsp_nsf_post", _ptr(x), _ptr(w), _ptr(b), int(B), T, C, int(K), float(slope), _ptr(out), _ptr(n_dev), int(scale))
        return out[0] if rows is None else out

    def stft_frames(self, audio, n_dev, n_fft, hop, L):
        """audio (B, T) with n_dev[b] samples per row (None: every row whole) -> frames (B, L, n_fft) padded per row as
        `STFT.get_mel` pads (reflect or zeros, chosen per row); frames past a row's own count are 0."""
        audio = audio.contiguous().float()
        B, T = audio.shape
        out = torch.empty(B, int(L), int(n_fft), device=audio.device, dtype=torch.float32)
        self.call("ddsp_stft_frames", _ptr(audio), B, T, _ptr(n_dev), int(n_fft), int(hop), int(L), _ptr(out))
        return out

    def nsf_mean(self, terms, want_out=True, act_slope=None, act_split=False):
        """Mean of up to three tensors -> out, or (out | None, leaky_relu(out, act_slope)) when act_slope is given
        (`act_split`: that copy in the split operand layout, see conv1d)."""
        a = terms[0]
        out = torch.empty_like(a) if want_out else None
        act = torch.empty_like(a) if act_slope is not None else None
        b = terms[1] if len(terms) > 1 else None
        c = terms[2] if len(terms) > 2 else None
        self.call("ddsp_nsf_mean", _ptr(a), _ptr(b), _ptr(c), len(terms), a.numel(), _ptr(out), _ptr(act),
                  float(act_slope if act_slope is not None else 1.0), CONV_ACT_SPLIT if act_split else 0)
        return out if act_slope is None else (out, act)

    def log_mel(self, frames, dft_table, mel_basis, clip):
        n_frames, n_fft = frames.shape
        n_mels = mel_basis.shape[0]
        out = torch.empty(n_frames, n_mels, device=frames.device, dtype=torch.float32)
        self.call("ddsp_log_mel", _ptr(frames), _ptr(dft_table), _ptr(mel_basis), n_frames, n_fft, n_mels, float(clip), _ptr(out))
        return out

    # -- a15 optimiser -------------------------------------------------------------------------
    def adamw_step(self, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step):
        self.call("ddsp_adamw_step", _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), float(lr),
                  float(beta1), float(beta2), float(eps), float(weight_decay), int(step))

    def adamw_step_multi(self, params, grads, exp_avgs, exp_avg_sqs, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
        """One AdamW update of a whole list of parameter tensors (shared hyper-parameters and step): the pointer
        tables go to the library as host arrays, the library issues one launch per 24 tensors.  grad_scale: every gradient is
        multiplied by it as it is read; exactly 1.0 runs the kernel that does not multiply."""
        if not _math.isfinite(float(grad_scale)):
            raise ValueError("adamw_step_multi: grad_scale must be finite")
        n = len(params)
        if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == n):
            raise ValueError("adamw_step_multi: lists of different length")
        for t in (*params, *grads, *exp_avgs, *exp_avg_sqs):
            if t.dtype != torch.float32:
                raise ValueError("adamw_step_multi: fp32 tensors only")
        for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
            if not (g.numel() == m.numel() == v.numel() == p.numel()):
                raise ValueError("adamw_step_multi: a tensor and its state differ in size")
        arr = lambda ts: (_vp * n)(*[_ptr(t) for t in ts])
        numel = (_i64 * n)(*[p.numel() for p in params])
        self.call("ddsp_adamw_step_multi", n, arr(params), arr(grads), arr(exp_avgs), arr(exp_avg_sqs), numel, float(lr), float(beta1),
                  float(beta2), float(eps), float(weight_decay), int(step), float(grad_scale))

    # -- building block ------------------------------------------------------------------------
    def gemm(self, A, B, bias=None, a_k_contig=True, b_k_contig=True, tile=0, variant=0, out=None):
        """C = op(A) @ op(B) (+bias): A (M,K) or (K,M) when not a_k_contig; B (N,K) or (K,N) when not b_k_contig.
        `out`: an (M, N) matrix to write into (the residual variants of the wave-specialised tiles ADD to it)."""
        M, K = (A.shape if a_k_contig else A.shape[::-1])
        N = B.shape[0] if b_k_contig else B.shape[1]
        C = torch.empty(M, N, device=A.device, dtype=torch.float32) if out is None else out
        if C.shape != (M, N) or C.dtype != torch.float32 or not C.is_contiguous():
            raise ValueError("gemm: `out` must be a contiguous fp32 (M, N) matrix")
        for t in (A, B):
            if not t.is_cuda or t.stride(1) != 1 or t.dtype != torch.float32:
                raise ValueError("gemm operands must be fp32 device matrices with unit inner stride")
        self.call("ddsp_gemm_f32", A.data_ptr(), A.stride(0), int(a_k_contig), B.data_ptr(), B.stride(0), int(b_k_contig),
                  _ptr(bias), _ptr(C), N, M, N, K, int(tile), int(variant))
        return C

    def performer_attention(self, q, k, v, proj, B, Fr, math=MATH_SPLIT_BF16):
        """q, k, v (B*Fr, 512), proj (266, 64) -> merged heads (B*Fr, 512) before `to_out` (pcmer.py:69-77,123-159)."""
        out = torch.empty(B * Fr, 512, device=q.device, dtype=torch.float32)
        self.call("ddsp_performer_attention", _ptr(q), _ptr(k), _ptr(v), _ptr(proj), int(B), int(Fr), _ptr(out), int(math))
        return out

    def softmax_attention(self, q, k, v, B, L, heads, math=MATH_SPLIT_BF16, n_keys_dev=None, out=None):
        """q, k, v (B*L, heads*64) -> softmax(q k^T / 8) v per (utterance, head), merged heads (B*L, heads*64), written into
        `out` when given.  `n_keys_dev` ((B,) int32 device tensor): utterance b attends over its first n_keys[b] rows only, and
        only those rows of `out` (given, or new and uninitialised) are written."""
        if out is None:
            out = torch.empty(B * L, heads * 64, device=q.device, dtype=torch.float32)
        elif out.dtype != torch.float32 or tuple(out.shape) != (B * L, heads * 64):
            raise ValueError("softmax_attention: `out` must be fp32 (B*L, heads*64)")
        self.call("ddsp_softmax_attention", _ptr(q), _ptr(k), _ptr(v), int(B), int(L), int(heads), _ptr(out), int(math),
                  _ptr(n_keys_dev))
        return out

    # -- units encoder -------------------------------------------------------------------------
    def hubert_units(self, weights, wav, n_dev=None):
        """weights: a HubertWeights struct; wav (B,T) 16 kHz fp32 -> units (B, Fr, 256).  n_dev: the (B,) int32 device tensor
        of a ragged batch's sample counts (`ragged_counts` of `check_hubert_n_samples`): every row as if encoded alone, 0
        after its own frames."""
        B, T = wav.shape
        Fr = hubert_frames(T)
        if Fr <= 0:
            raise ValueError(f"hubert: {T} samples are too short for the conv stack")
        wav = wav.contiguous().float()
        out = torch.empty(B, Fr, 256, device=wav.device, dtype=torch.float32)
        if B:
            self.call("ddsp_hubert_soft_units", ctypes.byref(weights), _ptr(wav), int(B), int(T), _ptr(n_dev), _ptr(out))
        return out

    def hubert_encode(self, weights, wav, layer, n_dev=None):
        """The conv stack's output (B, Fr, 512) for layer -1, else the hidden state (B, Fr, 768) after `layer` of the 12
        transformer layers.  n_dev: as in `hubert_units`."""
        B, T = wav.shape
        Fr = hubert_frames(T)
        if Fr <= 0:
            raise ValueError(f"hubert: {T} samples are too short for the conv stack")
        wav = wav.contiguous().float()
        out = torch.empty(B, Fr, 512 if layer == -1 else 768, device=wav.device, dtype=torch.float32)
        if B:
            self.call("ddsp_hubert_encode", ctypes.byref(weights), _ptr(wav), int(B), int(T), _ptr(n_dev), int(layer), _ptr(out))
        return out

    def hubert_base_units(self, weights, wav, n_layers=9, project=True, n_dev=None):
        """weights: a HubertBaseWeights struct; wav (B,T) 16 kHz fp32, not padded -> the hidden state after `n_layers` (1..12)
        transformer layers (B, Fr, 768), or with `project` its final projection (B, Fr, 256).  n_dev: as in `hubert_units`,
        the counts checked with `check_hubert_base_n_samples`."""
        B, T = wav.shape
        Fr = hubert_base_frames(T)
        if Fr <= 0:
            raise ValueError(f"hubert: {T} samples are too short for the conv stack")
        if not 1 <= int(n_layers) <= 12:
            raise ValueError("hubert_base_units: n_layers in 1..12")
        wav = wav.contiguous().float()
        out = torch.empty(B, Fr, 256 if project else 768, device=wav.device, dtype=torch.float32)
        if B:
            self.call("ddsp_hubert_base_units", ctypes.byref(weights), _ptr(wav), int(B), int(T), _ptr(n_dev), int(n_layers),
                      int(bool(project)), _ptr(out))
        return out

    # -- f0 extractor (CREPE) --------------------------------------------------------------------
    def crepe_activations(self, weights, audio16, hop=80, n_samples=None, counts_dev=None):
        """weights: a CrepeWeights struct; audio16 (B,T) 16 kHz fp32 -> sigmoid activations (B, 1 + T // hop, 360).
        `n_samples` (a sequence of B ints or a CPU integer tensor (B,)): a RAGGED batch - the network runs over the packed
        list of the rows' own 1 + n_samples[b] // hop frames only, row b is what the call returns for audio16[b, :n_samples[b]]
        alone and 0 after its frames, and what follows a row's samples is never read.  `counts_dev`: a caller that has
        already uploaded `crepe_ragged_table(n_samples, hop)` passes the (2B + 1,) int32 device tensor (one upload for a chain
        of ragged calls); None uploads it here."""
        B, T = audio16.shape
        Fr = crepe_frames(T, hop)
        x = audio16.contiguous().float()
        if n_samples is not None:
            vals = check_crepe_n_samples(n_samples, B, T, hop)
            table = crepe_ragged_table(vals, hop)
            if counts_dev is None:
                counts_dev = self.ragged_counts(table)
            elif counts_dev.dtype != torch.int32 or counts_dev.numel() != 2 * B + 1 or not counts_dev.is_contiguous():
                raise ValueError("crepe_activations: counts_dev must be the (2B + 1,) int32 upload of crepe_ragged_table")
        out = torch.empty(B, Fr, 360, device=x.device, dtype=torch.float32)
        ragged = (None, None, 0) if n_samples is None else (_ptr(counts_dev), _ptr(counts_dev) + 4 * B, int(table[-1]))
        if B:
            self.call("ddsp_crepe_activations", ctypes.byref(weights), _ptr(x), int(B), int(T), *ragged, int(hop), _ptr(out))
        return out

    def crepe_decode(self, probs, fmin, fmax, segment=512, dither_seed=0, dither=False, want_bins=False, seed_dev=None,
                     n_frames=None, counts_dev=None):
        """probs (B, Fr, 360) -> (f0 (B, Fr), periodicity (B, Fr)[, bins (B, Fr) int32]): the range mask, the Viterbi decode
        in independent pieces of `segment` frames (0: whole track), bins to Hz with the optional triangular dither.
        `seed_dev`: a (1,) int64 device tensor that holds the dither seed instead of `dither_seed` and is advanced to
        `next_dither_seed` of its value by the call (what a captured graph needs).
        `n_frames` (a sequence of B ints or a CPU integer tensor (B,)): a RAGGED batch - row b is decoded over its own
        n_frames[b] frames as a call on probs[b:b+1, :n_frames[b]] with the same seed decodes it, bit for bit, and every
        output is 0 after them.  `counts_dev`: the (B,) int32 device tensor of the same counts when the caller has
        uploaded them already (`ragged_counts`); None uploads them here."""
        p = probs.contiguous().float()
        B, Fr, _ = p.shape
        n_dev = None
        if n_frames is not None:
            if seed_dev is not None:
                raise ValueError("crepe_decode: seed_dev is not available with n_frames (a ragged batch)")
            vals = check_n_frames(n_frames, B, Fr)
            n_dev = self._counts_dev(counts_dev, B) if counts_dev is not None else self.ragged_counts(vals)
        f0 = torch.empty(B, Fr, device=p.device, dtype=torch.float32)
        pd = torch.empty_like(f0)
        bins = torch.empty(B, Fr, device=p.device, dtype=torch.int32) if want_bins else None
        if seed_dev is not None and (seed_dev.dtype != torch.int64 or seed_dev.numel() != 1 or seed_dev.device != p.device):
            raise ValueError("crepe_decode: seed_dev must be a (1,) int64 tensor on the device of probs")
        seed = int(dither_seed) & ((1 << 64) - 1)
        if B and Fr:
            self.call("ddsp_crepe_decode", _ptr(p), int(B), int(Fr), _ptr(n_dev), float(fmin), float(fmax), int(segment), seed,
                      _ptr(seed_dev), 1 if dither else 0, _ptr(f0), _ptr(pd), _ptr(bins))
        return (f0, pd, bins) if want_bins else (f0, pd)

    def f0_postfilter(self, f0, pd, sr, hop, n_frames, start_frame=0, threshold=0.05, uv_interp=False, f0_min=65.0,
                      n_crepe=None, n_out=None, counts_dev=None):
        """f0, pd (B, Fr) at the CREPE rate -> (B, n_frames): the reference's median / threshold / masked-average filter,
        re-timed to frames of `hop` samples at `sr` (a float hop keeps its fraction), `start_frame` zeros in front, and
        with uv_interp the numpy.interp fill of the zero frames and the clamp to f0_min (ddsp/vocoder.py:96-113).
        `n_crepe`, `n_out` (both or neither; sequences of B ints or CPU integer tensors (B,)): a RAGGED batch - row b has
        n_crepe[b] >= 3 CREPE frames and n_out[b] <= n_frames output frames of its own; its windows reflect at its own end,
        the fill looks at its own frames only, and the output is 0 after them.  start_frame must be 0.  `counts_dev`: the
        pair of (B,) int32 device tensors of the same counts when the caller has uploaded them already."""
        f0 = f0.contiguous().float()
        pd = pd.contiguous().float()
        B, Fr = f0.shape
        if pd.shape != f0.shape:
            raise ValueError("f0_postfilter: f0 and pd must have the same shape")
        if (n_crepe is None) != (n_out is None):
            raise ValueError("f0_postfilter: a ragged batch needs both n_crepe and n_out")
        nc = no = None
        if n_crepe is not None:
            if int(start_frame) != 0:
                raise ValueError("f0_postfilter: start_frame must be 0 with n_crepe / n_out (a ragged batch)")
            vals = []
            for name, c, lo, hi in (("n_crepe", n_crepe, 3, Fr), ("n_out", n_out, 1, int(n_frames))):
                vals.append(_check_counts(name, c, B))
                for b, v in enumerate(vals[-1]):
                    if not lo <= v <= hi:
                        raise ValueError(f"{name}[{b}] = {v} is outside {lo}..{hi}")
            if counts_dev is not None:
                nc, no = (self._counts_dev(c, B) for c in counts_dev)
            else:
                nc, no = self.ragged_counts(vals[0] + vals[1]).reshape(2, B)
        out = torch.empty(B, int(n_frames), device=f0.device, dtype=torch.float32)
        if B:
            self.call("ddsp_f0_postfilter", _ptr(f0), _ptr(pd), int(B), int(Fr), _ptr(nc), int(sr), float(hop), int(n_frames),
                      int(start_frame), _ptr(no), float(threshold), 1 if uv_interp else 0, float(f0_min), _ptr(out))
        return out

    def f0_ac(self, audio, sr, hop, f0_min, f0_max, n_frames, start_frame=0, uv_interp=False, n_dev=None, want_choice=False):
        """audio (B,T) at `sr` -> f0 (B, n_frames): the autocorrelation extractor (Boersma 1993 with the parameters of the
        reference's 'parselmouth' call), padded to `n_frames` frames of `hop` samples with `start_frame` extra zeros in front,
        and with uv_interp the numpy.interp fill of the unvoiced frames and the clamp to f0_min.  The caller has checked that
        T (every row of a ragged batch) holds one window (`f0_ac_frames(...) >= 1`).
        `n_dev` ((B,) int32 device tensor, `ragged_counts`): a RAGGED batch - row b is audio[b, :n[b]] analysed alone, with
        n[b] // hop + 1 frames and 0 after them; start_frame must be 0.  `want_choice`: also the chosen candidate of every
        analysis frame, (B, f0_ac_frames(T, ...)) int32, 0 = unvoiced."""
        audio = audio.contiguous().float()
        B, T = audio.shape
        if n_dev is not None and int(start_frame) != 0:
            raise ValueError("f0_ac: start_frame must be 0 with n_dev (a ragged batch)")
        out = torch.empty(B, int(n_frames), device=audio.device, dtype=torch.float32)
        choice = torch.empty(B, f0_ac_frames(T, sr, hop, f0_min), device=audio.device, dtype=torch.int32) if want_choice else None
        if B:
            n_dev = None if n_dev is None else self._counts_dev(n_dev, B)
            self.call("ddsp_f0_ac", _ptr(audio), int(B), int(T), _ptr(n_dev), int(sr), float(hop), float(f0_min), float(f0_max),
                      int(n_frames), int(start_frame), 1 if uv_interp else 0, _ptr(out), _ptr(choice))
        return (out, choice) if want_choice else out

    def slicer(self, x, win, hop, threshold, min_length, min_interval, max_sil_kept, pad_mode="constant", n_dev=None,
               capacity=None, out=None):
        """audio x (B,T) -> (table (B, capacity, 3) int32 rows start_sample, end_sample, is_silence; count (B,) int32; rms
        (B, slicer_frames(T, win, hop)) fp32): the reference's `Slicer.slice` per row - frame RMS over windows of `win`
        samples every `hop` (pad_mode "constant": librosa >= 0.10, "reflect": older), then its tagging state machine with the
        linear `threshold` and `min_length`, `min_interval`, `max_sil_kept` in frames.  Rows of the table from count[b] on
        are zeros.  `n_dev` ((B,) int32 device tensor, `ragged_counts`): a RAGGED batch - row b is x[b, :n[b]] cut alone.
        `capacity`: the table's rows, `slicer_capacity(...)` (always enough) when None; a row with more chunks than a smaller
        one keeps what fits and raises ValueError from `poll_error()` after a synchronise or from the next call.  `out`: a
        (table, count, rms) triple of preallocated contiguous tensors to write into.  Nothing is read back."""
        x = x.contiguous().float()
        B, T = x.shape
        F = slicer_frames(T, win, hop)
        cap = slicer_capacity(F, min_interval) if capacity is None else int(capacity)
        shapes = (((B, cap, 3), torch.int32), ((B,), torch.int32), ((B, F), torch.float32))
        if out is None:
            out = tuple(torch.empty(shape, device=x.device, dtype=dt) for shape, dt in shapes)
        else:
            for t, (shape, dt) in zip(out, shapes):
                if tuple(t.shape) != shape or t.dtype != dt:
                    raise ValueError(f"slicer: `out` must hold {dt} of shape {shape}, got {t.dtype} {tuple(t.shape)}")
        table, count, rms = out
        if pad_mode not in SLICER_PAD:
            raise ValueError(f"slicer: pad_mode must be one of {sorted(SLICER_PAD)}, got {pad_mode!r}")
        if B:
            n_dev = None if n_dev is None else self._counts_dev(n_dev, B)
            self.call("ddsp_slicer", _ptr(x), int(B), int(T), _ptr(n_dev), int(win), int(hop), float(threshold), int(min_length),
                      int(min_interval), int(max_sil_kept), SLICER_PAD[pad_mode], _ptr(rms), _ptr(table), _ptr(count), cap)
        return table, count, rms

    # -- a10 -----------------------------------------------------------------------------------
    def sins_bank(self, ctrl2d, col0, n_harmonics, f0_frames, phase, B, Fr, hop, sr):
        out = torch.empty(B, Fr * hop, device=ctrl2d.device, dtype=torch.float32)
        f0 = f0_frames.reshape(-1).contiguous().float()
        self.call("ddsp_sins_bank", _ptr(ctrl2d) + 4 * col0, ctrl2d.shape[-1], int(n_harmonics), _ptr(f0), _ptr(phase),
                  B, Fr, int(hop), int(sr), _ptr(out))
        return out

    # -- a11 -----------------------------------------------------------------------------------
    def spectral_ola(self, ctrl2d, comb, noise, excitation, noise_seed, B, Fr, hop):
        out = torch.empty(B, Fr * hop, device=ctrl2d.device, dtype=torch.float32)
        self.call("ddsp_spectral_ola", _ptr(ctrl2d), ctrl2d.shape[-1], _ptr(comb), _ptr(noise), int(excitation),
                  int(noise_seed), B, Fr, int(hop), _ptr(out))
        return out

    def sins_bank_bwd(self, ctrl2d, col0, n_harmonics, f0_frames, phase, d_out, B, Fr, hop, sr, d_ctrl2d):
        f0 = f0_frames.reshape(-1).contiguous().float()
        self.call("ddsp_sins_bank_bwd", _ptr(ctrl2d) + 4 * col0, ctrl2d.shape[-1], int(n_harmonics), _ptr(f0),
                  _ptr(phase), _ptr(d_out.contiguous()), B, Fr, int(hop), int(sr), _ptr(d_ctrl2d) + 4 * col0,
                  d_ctrl2d.shape[-1])

    def spectral_ola_bwd(self, ctrl2d, comb, noise, excitation, noise_seed, d_out, B, Fr, hop):
        d_ctrl = torch.empty_like(ctrl2d)
        self.call("ddsp_spectral_ola_bwd", _ptr(ctrl2d), ctrl2d.shape[-1], _ptr(comb), _ptr(noise), int(excitation),
                  int(noise_seed), _ptr(d_out.contiguous()), B, Fr, int(hop), _ptr(d_ctrl), d_ctrl.shape[-1])
        return d_ctrl

    # -- a13 -----------------------------------------------------------------------------------
    def rss_loss(self, x_pred, x_true, n_ffts, alpha=1.0, eps=1e-7, want_grad=False, hops=None, n_samples=None, rows=False,
                 global_n_samples=None):
        """-> (loss (1,) device tensor, d loss/d x_pred (B,T) | None) for the given list of scales; `hops`: one hop per
        scale (default: hop = n_fft, the reference's overlap = 0).  `n_samples`: the list `check_n_samples` returned -
        rows of different length (include/ddsp_amd.h: the counts of ddsp_rss_loss).  `rows` (with `n_samples`, without
        `want_grad`): -> (loss per row (B,), None), every row scored alone (ddsp_rss_loss_rows).  `global_n_samples` (with
        `n_samples`, without `rows`): the list `check_global_n_samples` returned - the rows are one rank's share of that
        global batch."""
        xp = x_pred.detach().contiguous().float()
        xt = x_true.detach().contiguous().float()
        B, T = xp.shape
        if xt.shape != xp.shape:
            raise ValueError(f"x_pred {tuple(xp.shape)} and x_true {tuple(xt.shape)} must have the same shape")
        if T % 4:
            raise ValueError("signal length must be a multiple of 4")
        if rows and (n_samples is None or want_grad):
            raise ValueError("rss_loss: rows=True takes n_samples and has no gradient")
        if global_n_samples is not None and (n_samples is None or rows):
            raise ValueError("rss_loss: global_n_samples takes n_samples and not rows=True")
        arr = (_int * len(n_ffts))(*[int(n) for n in n_ffts])
        if hops is not None and len(hops) != len(n_ffts):
            raise ValueError("one hop per scale")
        harr = (_int * len(n_ffts))(*[int(h) for h in hops]) if hops is not None else None
        loss = torch.empty(B if rows else 1, device=xp.device, dtype=torch.float32)
        grad = torch.empty_like(xp) if want_grad else None
        ns, n_dev = (None, None) if n_samples is None else ((_int * B)(*n_samples), self.ragged_counts(n_samples))
        scales = (arr, harr, len(n_ffts), float(alpha), float(eps), _ptr(loss))
        if rows:
            self.call("ddsp_rss_loss_rows", _ptr(xp), _ptr(xt), B, T, ns, _ptr(n_dev), *scales)
        else:
            gns, n_global = (None, 0) if global_n_samples is None else ((_int * len(global_n_samples))(*global_n_samples),
                                                                        len(global_n_samples))
            self.call("ddsp_rss_loss", _ptr(xp), _ptr(xt), B, T, ns, _ptr(n_dev), gns, n_global, *scales, _ptr(grad))
        return loss, grad

    def vc_f0_map(self, f0_frames, spk_id, lfo, n_frames=None):
        """Validation's conversion leg (`ddsp_vc_f0_map`): f0 (B, Fr[, 1]), spk_id (B[, 1]) int64 1-based and the table lfo
        (n_spk,) fp32, on the device -> (mapped f0 in f0's shape, target ids in spk_id's shape): target = (src + 1) % n_spk, 0
        becomes 1; f0 * -> exp(lfo[tgt] * ln(f0) / lfo[src]), 0 stays 0.  n_frames: the (B,) int32 device tensor of a ragged
        batch (`ragged_counts`) - frames past a row's count come out 0."""
        B = f0_frames.shape[0]
        if spk_id.dtype != torch.int64 or spk_id.numel() != B:
            raise ValueError("vc_f0_map: spk_id must hold B int64 ids")
        if lfo.dtype != torch.float32 or lfo.dim() != 1 or lfo.numel() < 1:
            raise ValueError("vc_f0_map: lfo must be an fp32 table (n_spk,)")
        f0 = f0_frames.reshape(B, -1).contiguous().float()
        Fr = f0.shape[1]
        if n_frames is not None:
            self._counts_dev(n_frames, B)
        out = torch.empty_like(f0)
        tgt = torch.empty(B, device=f0.device, dtype=torch.int64)
        self.call("ddsp_vc_f0_map", _ptr(f0), _ptr(spk_id.contiguous()), _ptr(lfo.contiguous()), lfo.numel(), B, Fr, _ptr(n_frames),
                  _ptr(out), _ptr(tgt))
        return out.reshape(f0_frames.shape), tgt.reshape(spk_id.shape)

    # -- a14 -----------------------------------------------------------------------------------
    def sola(self, audio, sola_buffer, block, xfade, search, delay):
        """audio (N,), sola_buffer (xfade,) updated in place -> (emitted (block,), shift int32 device tensor).
        S streams: audio (S, N), sola_buffer (S, xfade) -> (emitted (S, block), shift (S,)); row s is the solo call on row s."""
        audio = audio.contiguous().float()
        rows = audio.dim() == 2
        S, n_audio = audio.shape if rows else (1, audio.numel())
        if rows and (tuple(sola_buffer.shape) != (S, int(xfade)) or sola_buffer.dtype != torch.float32):
            raise ValueError(f"sola: {S} streams need an fp32 sola_buffer (S, xfade) = {(S, int(xfade))}")
        emitted = torch.empty((S, int(block)) if rows else (block,), device=audio.device, dtype=torch.float32)
        shift = torch.empty(S, device=audio.device, dtype=torch.int32)
        self.call("ddsp_sola", _ptr(audio), S, n_audio, int(block), int(xfade), int(search), int(delay), _ptr(sola_buffer),
                  _ptr(emitted), _ptr(shift))
        return emitted, shift

    def stream_push_(self, window, block_in):
        """In place: window (n_in,) = append(window[block:], block_in (block,)) (gui.py:373-374); the window keeps its
        address (`ddsp_stream_push`).  S streams: windows (S, n_in) take blocks (S, block), every row like the solo call."""
        if window.dtype == torch.float32 and block_in.dtype == torch.float32 and window.dim() == 2:
            if block_in.dim() != 2 or block_in.shape[0] != window.shape[0]:
                raise ValueError("stream_push_: (S, n_in) windows take (S, block) blocks")
        elif window.dtype != torch.float32 or block_in.dtype != torch.float32 or window.dim() != 1 or block_in.dim() != 1:
            raise ValueError("stream_push_: window and block_in must be 1-D fp32 tensors")
        self.call("ddsp_stream_push", _ptr(window), window.shape[0] if window.dim() == 2 else 1, window.shape[-1], _ptr(block_in),
                  block_in.shape[-1])
        return window

    def bank_gather_(self, rows, block_in, windows, cwindows, sola_buffer, csola, mix, cmix, pitch, cpitch, request=None,
                     crequest=None):
        """The active set of a stream bank into its compact rows (`ddsp_bank_gather`): rows (W,) int32 device, entry r the slot
        of compact row r or -1 for padding.  In place: windows (S, n_in)[rows[r]] takes block_in (W, block)[r]; then cwindows
        (W, n_in), csola (W, xfade), cmix = (ids (W, K) int32, w (W, K)), cpitch (W,) and crequest (W,) int32 take the rows of
        windows, sola_buffer (S, xfade), mix, pitch (S,) and request (S,) int32 (both None: a bank without an enhancer).  A
        padding row gets zeros, speaker 1 with weight 1, pitch 1, request 0.  -> cwindows."""
        W, (S, n_in) = rows.numel(), windows.shape
        K = check_mix_rows(mix[0], mix[1], S)
        shapes = ((rows, (W,)), (block_in, (W, block_in.shape[-1])), (cwindows, (W, n_in)), (sola_buffer, (S, sola_buffer.shape[-1])),
                  (csola, (W, sola_buffer.shape[-1])), (pitch, (S,)), (cpitch, (W,)))
        if rows.dtype != torch.int32 or windows.dim() != 2 or any(tuple(t.shape) != s for t, s in shapes) or check_mix_rows(*cmix, W) != K:
            raise ValueError("bank_gather_: S rows of the bank, W compact rows and a (W,) int32 row table")
        if any(t.dtype != torch.float32 for t in (block_in, windows, cwindows, sola_buffer, csola, pitch, cpitch)):
            raise ValueError("bank_gather_: windows, blocks, buffers and pitch must be fp32")
        if (request is None) != (crequest is None) or (request is not None and (
                request.dtype != torch.int32 or crequest.dtype != torch.int32 or tuple(request.shape) != (S,) or tuple(crequest.shape) != (W,))):
            raise ValueError("bank_gather_: request (S,) and crequest (W,) int32, or neither")
        self.call("ddsp_bank_gather", _ptr(rows), W, S, _ptr(windows), n_in, _ptr(block_in), block_in.shape[-1], _ptr(cwindows),
                  _ptr(sola_buffer), sola_buffer.shape[-1], _ptr(csola), _ptr(mix[0]), _ptr(mix[1]), K, _ptr(cmix[0]), _ptr(cmix[1]),
                  _ptr(pitch), _ptr(cpitch), _ptr(request), _ptr(crequest))
        return cwindows

    def bank_scatter_(self, rows, csola, sola_buffer):
        """After the splice of the compact rows (`ddsp_bank_scatter`): sola_buffer (S, xfade)[rows[r]] = csola (W, xfade)[r] for
        every row of rows (W,) int32 that is no padding.  -> sola_buffer."""
        W, xfade = csola.shape
        if rows.dtype != torch.int32 or tuple(rows.shape) != (W,) or sola_buffer.dim() != 2 or sola_buffer.shape[1] != xfade:
            raise ValueError("bank_scatter_: csola (W, xfade), sola_buffer (S, xfade) and a (W,) int32 row table")
        if csola.dtype != torch.float32 or sola_buffer.dtype != torch.float32:
            raise ValueError("bank_scatter_: the buffers must be fp32")
        self.call("ddsp_bank_scatter", _ptr(rows), W, sola_buffer.shape[0], _ptr(csola), xfade, _ptr(sola_buffer))
        return sola_buffer

    def bank_glide_(self, rows, clock, bp_n, bp_t, bp_w, spk_w, w_frames, n_in, block, hop):
        """The per-frame mix weights of one call's rows from the slots' glide state, and the advance of those slots' clocks
        (`ddsp_bank_glide`): rows (W,) int32 device, entry r the slot of row r (anything outside [0, S): a padding row, weights
        (1, 0, ...)), or None for row r = slot r (W is then w_frames' row count).  In place: w_frames (W, Fr, K) takes, for frame
        t of a real row, the slot's breakpoints bp_t (S, P_max) int64 / bp_w (S, P_max, K) - the first bp_n (S,) int32 of them -
        interpolated at tau = clock[s] + block - n_in + t * hop, or spk_w (S, K) when the slot has none; then clock (S,) int64
        advances by `block` for the named slots alone.  No slot may be named twice.  -> w_frames."""
        if not (isinstance(w_frames, torch.Tensor) and w_frames.dim() == 3 and isinstance(clock, torch.Tensor) and clock.dim() == 1 and
                isinstance(bp_t, torch.Tensor) and bp_t.dim() == 2):
            raise ValueError("bank_glide_: w_frames (W, Fr, K), clock (S,) and bp_t (S, P_max)")
        (W, Fr, K), S, P_max = w_frames.shape, clock.numel(), bp_t.shape[1]
        tables = ((clock, torch.int64, (S,)), (bp_n, torch.int32, (S,)), (bp_t, torch.int64, (S, P_max)),
                  (bp_w, torch.float32, (S, P_max, K)), (spk_w, torch.float32, (S, K)), (w_frames, torch.float32, (W, Fr, K)))
        if rows is not None:
            tables += ((rows, torch.int32, (W,)),)
        if any(not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or
               t.device != w_frames.device for t, dtype, shape in tables):
            raise ValueError("bank_glide_: contiguous tensors on one device: clock (S,) int64, bp_n (S,) int32, bp_t (S, P_max) int64, "
                             "bp_w (S, P_max, K) fp32, spk_w (S, K) fp32, w_frames (W, Fr, K) fp32 and rows (W,) int32 or None")
        if not (1 <= K <= MAX_MIX and 1 <= P_max <= 64 and S >= 1 and Fr >= 1 and W <= 65535 and int(block) >= 1 and int(n_in) >= 1 and
                float(hop) > 0):
            raise ValueError(f"bank_glide_: 1 <= K <= {MAX_MIX}, 1 <= P_max <= 64, W <= 65535, Fr, block, n_in >= 1 and hop > 0")
        if W:
            self.call("ddsp_bank_glide", _ptr(rows), W, S, _ptr(clock), _ptr(bp_n), _ptr(bp_t), _ptr(bp_w), P_max, _ptr(spk_w), K, Fr,
                      int(n_in), int(block), float(hop), _ptr(w_frames))
        return w_frames

    def bank_key_glide_(self, rows, key_clock, key_n, key_t, key_semi, key_fac, pitch, pitch_frames, n_in, block, hop):
        """The per-frame f0 factors of one call's rows from the slots' key timelines, and the advance of those slots' key clocks
        (`ddsp_bank_key_glide`): `bank_glide_` with a key timeline in place of the weights.  rows (W,) int32 device or None as
        there.  In place: pitch_frames (W, Fr) takes, for frame t of a real row, the slot's breakpoints key_t (S, P_max) int64 /
        key_semi, key_fac (S, P_max) fp32 - the first key_n (S,) int32 of them - at tau = key_clock[s] + block - n_in + t * hop
        by the key timeline rule (include/ddsp_amd.h), or pitch (S,)[s] when the slot has none, 1.0 on a padding row; then
        key_clock (S,) int64 advances by `block` for the named slots alone.  No slot may be named twice.  -> pitch_frames."""
        if not (isinstance(pitch_frames, torch.Tensor) and pitch_frames.dim() == 2 and isinstance(key_clock, torch.Tensor) and
                key_clock.dim() == 1 and isinstance(key_t, torch.Tensor) and key_t.dim() == 2):
            raise ValueError("bank_key_glide_: pitch_frames (W, Fr), key_clock (S,) and key_t (S, P_max)")
        (W, Fr), S, P_max = pitch_frames.shape, key_clock.numel(), key_t.shape[1]
        tables = ((key_clock, torch.int64, (S,)), (key_n, torch.int32, (S,)), (key_t, torch.int64, (S, P_max)),
                  (key_semi, torch.float32, (S, P_max)), (key_fac, torch.float32, (S, P_max)), (pitch, torch.float32, (S,)),
                  (pitch_frames, torch.float32, (W, Fr)))
        if rows is not None:
            tables += ((rows, torch.int32, (W,)),)
        if any(not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or
               t.device != pitch_frames.device for t, dtype, shape in tables):
            raise ValueError("bank_key_glide_: contiguous tensors on one device: key_clock (S,) int64, key_n (S,) int32, key_t "
                             "(S, P_max) int64, key_semi, key_fac (S, P_max) fp32, pitch (S,) fp32, pitch_frames (W, Fr) fp32 and "
                             "rows (W,) int32 or None")
        if not (1 <= P_max <= 64 and S >= 1 and Fr >= 1 and W <= 65535 and int(block) >= 1 and int(n_in) >= 1 and float(hop) > 0):
            raise ValueError("bank_key_glide_: 1 <= P_max <= 64, W <= 65535, Fr, block, n_in >= 1 and hop > 0")
        if W:
            self.call("ddsp_bank_key_glide", _ptr(rows), W, S, _ptr(key_clock), _ptr(key_n), _ptr(key_t), _ptr(key_semi),
                      _ptr(key_fac), P_max, _ptr(pitch), Fr, int(n_in), int(block), float(hop), _ptr(pitch_frames))
        return pitch_frames

    def ctrl_warp_(self, ctrl2d, segments, factor, Fr, slot_of_row=None, n_dev=None):
        """The formant shift (`ddsp_ctrl_warp`; include/ddsp_amd.h states the rule): in place on the control matrix ctrl2d
        (rows, sum) fp32, rows = B * Fr, up to three `segments` (first column, n, origin) - origin 0: magnitude bins, 1: harmonics -
        are read at f / factor.  factor: fp32 device FACTORS, (B * Fr,) or (B, Fr) one per frame, (B,) one per batch row, or
        - with slot_of_row (B,) int32 device - (S,) read as factor[slot_of_row[b]], an entry outside [0, S) being a padding row
        (factor 1).  n_dev (B,) int32 device: the counts of a ragged batch, frames at or past them keep their bits.  Shapes and
        dtypes are refused here, before the launch; a factor that is not finite or not > 0 leaves its row as it was and raises
        ValueError from `poll_error()` after a synchronise or from the next call that takes the error word.  -> ctrl2d."""
        if not (isinstance(ctrl2d, torch.Tensor) and ctrl2d.dtype == torch.float32 and ctrl2d.dim() == 2 and ctrl2d.is_contiguous()):
            raise ValueError("ctrl_warp_: ctrl2d must be a contiguous (rows, sum) fp32 tensor")
        rows, width = ctrl2d.shape
        Fr = int(Fr)
        if Fr < 1 or rows % Fr:
            raise ValueError(f"ctrl_warp_: rows = {rows} must be a multiple of Fr = {Fr} >= 1")
        B = rows // Fr
        segments = [tuple(seg) for seg in segments] if isinstance(segments, (list, tuple)) else None
        if not segments or len(segments) > 3 or any(len(seg) != 3 or any(isinstance(v, bool) or not isinstance(v, int) for v in seg)
                                                    for seg in segments):
            raise ValueError("ctrl_warp_: segments is a list of 1 to 3 triples (first column, n, origin) of ints")
        for first, n, origin in segments:
            if not (first >= 0 and 1 <= n <= 4096 and first + n <= width and origin in (0, 1)):
                raise ValueError(f"ctrl_warp_: segment {(first, n, origin)} must lie inside the row of {width} columns with "
                                 "1 <= n <= 4096 and origin 0 or 1")
        if not (isinstance(factor, torch.Tensor) and factor.dtype == torch.float32 and factor.is_contiguous() and
                factor.device == ctrl2d.device):
            raise ValueError("ctrl_warp_: factor must be a contiguous fp32 tensor on the matrix's device")
        S = 0
        if slot_of_row is not None:
            if not (isinstance(slot_of_row, torch.Tensor) and slot_of_row.dtype == torch.int32 and tuple(slot_of_row.shape) == (B,)
                    and slot_of_row.is_contiguous() and slot_of_row.device == ctrl2d.device):
                raise ValueError(f"ctrl_warp_: slot_of_row must be a contiguous (B = {B},) int32 tensor on the matrix's device")
            if factor.dim() != 1 or factor.numel() < 1:
                raise ValueError("ctrl_warp_: with slot_of_row the factors are (S,), one per slot, S >= 1")
            per_frame, S = 0, factor.numel()
        elif tuple(factor.shape) in ((rows,), (B, Fr)) and Fr > 1:
            per_frame = 1
        elif tuple(factor.shape) == (B,):
            per_frame = 0
        elif tuple(factor.shape) == (B, 1):         # (Fr == 1: a factor per frame is a factor per row)
            per_frame = 0
        else:
            raise ValueError(f"ctrl_warp_: factor must be (B * Fr,) = ({rows},), (B, Fr) = ({B}, {Fr}) or (B,) = ({B},), got "
                             f"{tuple(factor.shape)}")
        if n_dev is not None and not (isinstance(n_dev, torch.Tensor) and n_dev.dtype == torch.int32 and n_dev.numel() == B and
                                      n_dev.is_contiguous() and n_dev.device == ctrl2d.device):
            raise ValueError(f"ctrl_warp_: n_dev must be a contiguous (B = {B},) int32 tensor on the matrix's device")
        if rows:
            table = (_c.c_int32 * (3 * len(segments)))(*[int(v) for seg in segments for v in seg])
            self.call("ddsp_ctrl_warp", _ptr(ctrl2d), rows, width, table, len(segments), _ptr(factor), per_frame, Fr,
                      _ptr(slot_of_row), S, _ptr(n_dev))
        return ctrl2d

    def f0_tune_(self, f0, mask, param, n_frames=None, owner=None, corr=None):
        """Pitch correction (`ddsp_f0_tune`; include/ddsp_amd.h states the rule): in place on f0, fp32 (B, Fr) or (B, Fr, 1), every
        voiced frame is pulled toward the nearest note that its owner's setting allows.  All device tensors: mask (J,) int32 and
        param (J, 3) fp64 (a4, strength, alpha) are the J settings (`infer_offline.PitchTune.setting`); owner (B,) int32 names
        the setting of every row - one outside [0, J) is a padding row, left as it is -, None: row b takes setting b; n_frames (B,)
        int32: the counts of a ragged batch; corr (B, Fr) fp64: receives the correction c_t in semitones, 0 where nothing is
        corrected.  Shapes, dtypes and devices are refused here, before the launch; a bad setting leaves its rows as they were
        and raises ValueError from `poll_error()` after a synchronise or from the next call that takes the error word.  -> f0."""
        if not (isinstance(f0, torch.Tensor) and f0.dtype == torch.float32 and f0.is_contiguous() and f0.is_cuda and
                (f0.dim() == 2 or (f0.dim() == 3 and f0.shape[2] == 1)) and f0.shape[0] >= 1 and f0.shape[1] >= 1):
            raise ValueError("f0_tune_: f0 must be a contiguous (B, Fr) or (B, Fr, 1) fp32 device tensor with B, Fr >= 1")
        B, Fr = int(f0.shape[0]), int(f0.shape[1])

        def on_device(t, dtype, shape):
            return isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and \
                t.device == f0.device

        if not (isinstance(mask, torch.Tensor) and mask.dim() == 1 and mask.numel() >= 1 and on_device(mask, torch.int32, tuple(mask.shape))):
            raise ValueError("f0_tune_: mask must be a contiguous (J,) int32 tensor on f0's device, J >= 1")
        J = int(mask.numel())
        if not on_device(param, torch.float64, (J, 3)):
            raise ValueError(f"f0_tune_: param must be a contiguous (J = {J}, 3) fp64 tensor on f0's device")
        if n_frames is not None and not on_device(n_frames, torch.int32, (B,)):
            raise ValueError(f"f0_tune_: n_frames must be a contiguous (B = {B},) int32 tensor on f0's device")
        if owner is not None and not on_device(owner, torch.int32, (B,)):
            raise ValueError(f"f0_tune_: owner must be a contiguous (B = {B},) int32 tensor on f0's device")
        if corr is not None and not on_device(corr, torch.float64, (B, Fr)):
            raise ValueError(f"f0_tune_: corr must be a contiguous (B = {B}, Fr = {Fr}) fp64 tensor on f0's device")
        self.call("ddsp_f0_tune", _ptr(f0), B, Fr, _ptr(n_frames), _ptr(owner), J, _ptr(mask), _ptr(param), _ptr(corr))
        return f0

    def units_index_norms(self, vec):
        """nrm (N,) fp32 = the squared norms of the index entries vec (N, C) fp32 (`ddsp_units_index_norms`): the derived row of
        an index, formed once when it goes up."""
        if not (isinstance(vec, torch.Tensor) and vec.dtype == torch.float32 and vec.dim() == 2 and vec.is_cuda and
                vec.is_contiguous() and vec.shape[0] >= 1 and 4 <= vec.shape[1] <= 1024 and vec.shape[1] % 4 == 0):
            raise ValueError("units_index_norms: vec must be a contiguous (N, C) fp32 device tensor, N >= 1, C a multiple of 4 in 4..1024")
        nrm = torch.empty(vec.shape[0], dtype=torch.float32, device=vec.device)
        self.call("ddsp_units_index_norms", _ptr(vec), int(vec.shape[0]), int(vec.shape[1]), _ptr(nrm))
        return nrm

    def units_retrieve_workspace(self, rows, Fr, k, N_max):
        """Bytes of the workspace of a `units_retrieve_` call of this shape (`ddsp_units_retrieve_workspace`)."""
        n = _i64()
        self._check(self.lib.ddsp_units_retrieve_workspace(self.handle, int(rows), int(Fr), int(k), int(N_max), ctypes.byref(n)),
                    "ddsp_units_retrieve_workspace")
        return int(n.value)

    def units_retrieve_(self, units, bank, index_of_row, ratio_of_row, k=8, n_frames=None, nn_id=None, nn_dist=None, owner=None):
        """Unit retrieval (`ddsp_units_retrieve`; include/ddsp_amd.h states the rule): in place on units (rows, Fr, C) fp32, every
        frame of a row that names an index is blended with the weighted mean of its k nearest entries of that index.  bank: an
        `infer_offline.UnitIndexBank` on units' device (off, vec, nrm, `workspace(rows, Fr, k)`); index_of_row (rows,) int32 - -1
        or anything outside [0, X): none, the row keeps its bits -, ratio_of_row (rows,) fp32 in [0, 1]; n_frames (rows,) int32:
        the counts of a ragged batch; nn_id (rows, Fr, k) int32 and nn_dist (rows, Fr, k) fp32 receive the selected entry ids
        (-1: unused) and their squared distances.  owner (rows,) int32: index_of_row and ratio_of_row are then J SETTINGS (a
        bank's slots) and row b takes setting owner[b] - one outside [0, J) is a padding row, left as it is.  Shapes, dtypes and devices are refused here, before the launch; a bad ratio
        leaves its row as it was and raises ValueError from `poll_error()` after a synchronise or from the next call that
        takes the error word.  -> units."""
        if not (isinstance(units, torch.Tensor) and units.dtype == torch.float32 and units.dim() == 3 and units.is_cuda and
                units.is_contiguous() and units.shape[0] >= 1 and units.shape[1] >= 1):
            raise ValueError("units_retrieve_: units must be a contiguous (rows, Fr, C) fp32 device tensor with rows, Fr >= 1")
        rows, Fr, C = (int(n) for n in units.shape)
        if not all(hasattr(bank, a) for a in ("off", "vec", "nrm", "n_max", "workspace")):
            raise ValueError(f"units_retrieve_: bank must be an infer_offline.UnitIndexBank, got {type(bank).__name__}")
        if bank.vec.device != units.device or int(bank.vec.shape[1]) != C:
            raise ValueError(f"units_retrieve_: the bank holds {int(bank.vec.shape[1])} channels on {bank.vec.device}, units has "
                             f"{C} on {units.device}")
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_RETRIEVE_K:
            raise ValueError(f"units_retrieve_: k must be an int in 1..{MAX_RETRIEVE_K}, got {k!r}")

        def on_device(t, dtype, shape):
            return isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and \
                t.device == units.device

        if owner is not None and not on_device(owner, torch.int32, (rows,)):
            raise ValueError(f"units_retrieve_: owner must be a contiguous (rows = {rows},) int32 tensor on units' device")
        J = int(index_of_row.numel()) if isinstance(index_of_row, torch.Tensor) and owner is not None else rows
        if J < 1 or not on_device(index_of_row, torch.int32, (J,)):
            raise ValueError(f"units_retrieve_: index_of_row must be a contiguous ({J},) int32 tensor on units' device (one per row, "
                             f"or one per setting with owner=)")
        if not on_device(ratio_of_row, torch.float32, (J,)):
            raise ValueError(f"units_retrieve_: ratio_of_row must be a contiguous ({J},) fp32 tensor on units' device")
        if n_frames is not None and not on_device(n_frames, torch.int32, (rows,)):
            raise ValueError(f"units_retrieve_: n_frames must be a contiguous (rows = {rows},) int32 tensor on units' device")
        if nn_id is not None and not on_device(nn_id, torch.int32, (rows, Fr, k)):
            raise ValueError(f"units_retrieve_: nn_id must be a contiguous ({rows}, {Fr}, k = {k}) int32 tensor on units' device")
        if nn_dist is not None and not on_device(nn_dist, torch.float32, (rows, Fr, k)):
            raise ValueError(f"units_retrieve_: nn_dist must be a contiguous ({rows}, {Fr}, k = {k}) fp32 tensor on units' device")
        ws = bank.workspace(rows, Fr, k)                  # (the bank's own, allocated at construction for its declared shape)
        self.call("ddsp_units_retrieve", _ptr(units), rows, Fr, C, _ptr(n_frames), _ptr(owner), J, _ptr(index_of_row),
                  _ptr(ratio_of_row), int(bank.off.numel()) - 1, _ptr(bank.off), _ptr(bank.vec), _ptr(bank.nrm), int(bank.vec.shape[0]), int(bank.n_max),
                  k, _ptr(ws), int(ws.numel()) * ws.element_size(), _ptr(nn_id), _ptr(nn_dist))
        return units

    # -- the envelope mix ------------------------------------------------------------------------
    @staticmethod
    def _envelope_rows(name, x, counts, spans, n_max):
        """The checks the two envelope calls share -> (form, R, width): x is the MATRIX form - fp32 (R, T) with counts (R,) int32
        or None - or the SPANS form - fp64 (total,) with spans (R, 2) int64 and n_max, the longest count, a host int."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.is_contiguous() and x.numel() >= 1):
            raise ValueError(f"{name}: the signal must be a contiguous, non-empty device tensor")

        def on_device(t, dtype, shape):
            return isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and \
                t.device == x.device

        if x.dtype == torch.float32 and x.dim() == 2:
            if spans is not None or n_max is not None:
                raise ValueError(f"{name}: an fp32 (R, T) matrix takes counts, not spans")
            R, T = int(x.shape[0]), int(x.shape[1])
            if counts is not None and not on_device(counts, torch.int32, (R,)):
                raise ValueError(f"{name}: the counts must be a contiguous (R = {R},) int32 tensor on the signal's device")
            form, width = "matrix", T
        elif x.dtype == torch.float64 and x.dim() == 1:
            if counts is not None:
                raise ValueError(f"{name}: an fp64 tensor takes spans, not counts")
            if not (isinstance(spans, torch.Tensor) and spans.dim() == 2 and on_device(spans, torch.int64, (spans.shape[0], 2))
                    and spans.shape[0] >= 1):
                raise ValueError(f"{name}: spans must be a contiguous (R, 2) int64 tensor of (base, count) on the signal's device")
            if isinstance(n_max, bool) or not isinstance(n_max, int) or not 1 <= n_max <= x.numel():
                raise ValueError(f"{name}: n_max, the longest span, must be an int in 1..{x.numel()}, got {n_max!r}")
            form, R, width = "spans", int(spans.shape[0]), n_max
        else:
            raise ValueError(f"{name}: the signal must be an fp32 (R, T) matrix or an fp64 (total,) tensor with spans")
        if not 1 <= R <= 65535:
            raise ValueError(f"{name}: 1 to 65535 rows, got {R}")
        return form, R, width

    @staticmethod
    def _envelope_hop(name, what, hop):
        if isinstance(hop, bool) or not isinstance(hop, int) or not 1 <= hop <= 2 ** 27:
            raise ValueError(f"{name}: {what} must be an int in 1..2**27, got {hop!r}")
        return hop

    def envelope_rms(self, x, hop, m=2, n_samples=None, spans=None, n_max=None):
        """Frame RMS of ragged rows (`ddsp_envelope_rms`; include/ddsp_amd.h states the rule: librosa.feature.rms with
        center=True, 'constant' padding, win = m * hop) -> env (R, N_max) fp64, N = 1 + n // hop frames per row and 0 behind them.
        x: fp32 (R, T) with n_samples (R,) int32 device or None (N_max = 1 + T // hop), or fp64 (total,) with spans (R, 2) int64
        device rows of (base, count) and n_max, the longest count as a host int (N_max = 1 + n_max // hop).  m: 2, 4, 6 or 8.
        Shapes, dtypes, devices, m and hop are refused here, before the launch; a span that leaves the tensor or exceeds n_max
        gets a zero envelope and raises ValueError from `poll_error()` or the next call that takes the error word."""
        form, R, width = self._envelope_rows("envelope_rms", x, n_samples, spans, n_max)
        hop = self._envelope_hop("envelope_rms", "hop", hop)
        if isinstance(m, bool) or m not in (2, 4, 6, 8):
            raise ValueError(f"envelope_rms: m must be 2, 4, 6 or 8 (win = m * hop), got {m!r}")
        N_max = 1 + width // hop
        blocks = torch.empty(R, N_max, dtype=torch.float64, device=x.device)
        env = torch.empty(R, N_max, dtype=torch.float64, device=x.device)
        if form == "matrix":
            self.call("ddsp_envelope_rms", _ptr(x), width, _ptr(n_samples), None, 0, None, R, hop, m, N_max, _ptr(blocks), _ptr(env))
        else:
            self.call("ddsp_envelope_rms", None, 0, None, _ptr(x), int(x.numel()), _ptr(spans), R, hop, m, N_max, _ptr(blocks),
                      _ptr(env))
        return env

    def envelope_mix_(self, out, src, rate, env_out, hop_out, hop_src, src_samples, n_out=None, spans=None, n_max=None,
                      src_of_row=None, owner=None):
        """The envelope mix (`ddsp_envelope_apply`; include/ddsp_amd.h states the rule, RVC's `change_rms`): in place on the rows
        of `out`, out[t] *= e1^(1 - rate) * max(e2, 1e-6)^(rate - 1) with both envelopes interpolated to the row's length.
        out: fp32 (R, T) with n_out (R,) int32 or None, or fp64 (total,) with spans (R, 2) int64 and n_max (`envelope_rms`'s forms);
        env_out (R, >= 1 + width // hop_out) fp64: `envelope_rms` of `out` at hop_out; src (R_src, N_src) fp64: `envelope_rms` of
        the SOURCE rows at hop_src; src_samples: the sources' counts, (R_src,) int32 device or one host int for all; src_of_row
        (R,) int32 or None (row r's source is row r); rate (J,) fp64 device; owner (R,) int32 names the rate of every row (-1: a
        padding row, left alone) or None (row r takes rate r).  Rows with rate == 1 keep their bits.  Shapes, dtypes, devices
        and hops are refused here, before the launch; a bad rate, owner, source or span leaves its row and raises ValueError from
        `poll_error()` or the next call that takes the error word.  -> out."""
        form, R, width = self._envelope_rows("envelope_mix_", out, n_out, spans, n_max)
        hop_out = self._envelope_hop("envelope_mix_", "hop_out", hop_out)
        hop_src = self._envelope_hop("envelope_mix_", "hop_src", hop_src)

        def on_device(t, dtype, shape):
            return isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and \
                t.device == out.device

        if not (isinstance(env_out, torch.Tensor) and env_out.dim() == 2 and on_device(env_out, torch.float64, (R, env_out.shape[1]))
                and env_out.shape[1] >= 1 + width // hop_out):
            raise ValueError(f"envelope_mix_: env_out must be a contiguous (R = {R}, >= {1 + width // hop_out}) fp64 tensor on out's "
                             f"device (`envelope_rms` of out at hop_out)")
        if not (isinstance(src, torch.Tensor) and src.dim() == 2 and src.shape[0] >= 1 and src.shape[1] >= 1 and
                on_device(src, torch.float64, tuple(src.shape))):
            raise ValueError("envelope_mix_: src must be a contiguous (R_src, N_src) fp64 tensor on out's device (`envelope_rms` of "
                             "the source rows at hop_src)")
        R_src, N_src = int(src.shape[0]), int(src.shape[1])
        if isinstance(src_samples, torch.Tensor):
            if not on_device(src_samples, torch.int32, (R_src,)):
                raise ValueError(f"envelope_mix_: src_samples must be a contiguous (R_src = {R_src},) int32 tensor on out's device")
            n_src, n_src_all = src_samples, 0
        else:
            if isinstance(src_samples, bool) or not isinstance(src_samples, int) or src_samples < 1 or \
                    1 + src_samples // hop_src > N_src:
                raise ValueError(f"envelope_mix_: src_samples must be a device tensor of counts or an int >= 1 whose frames "
                                 f"src holds, got {src_samples!r}")
            n_src, n_src_all = None, src_samples
        if not (isinstance(rate, torch.Tensor) and rate.dim() == 1 and rate.numel() >= 1 and
                on_device(rate, torch.float64, tuple(rate.shape))):
            raise ValueError("envelope_mix_: rate must be a contiguous (J,) fp64 tensor on out's device, J >= 1")
        if src_of_row is not None and not on_device(src_of_row, torch.int32, (R,)):
            raise ValueError(f"envelope_mix_: src_of_row must be a contiguous (R = {R},) int32 tensor on out's device")
        if owner is not None and not on_device(owner, torch.int32, (R,)):
            raise ValueError(f"envelope_mix_: owner must be a contiguous (R = {R},) int32 tensor on out's device")
        tail = (R, width, _ptr(env_out), int(env_out.shape[1]), hop_out, _ptr(src), R_src, N_src, hop_src, _ptr(n_src), n_src_all,
                _ptr(src_of_row), _ptr(owner), _ptr(rate), int(rate.numel()))
        if form == "matrix":
            self.call("ddsp_envelope_apply", None, 0, None, _ptr(out), width, _ptr(n_out), *tail)
        else:
            self.call("ddsp_envelope_apply", _ptr(out), int(out.numel()), _ptr(spans), None, 0, None, *tail)
        return out

    @staticmethod
    def _kmeans_shapes(name, vec, cen, others):
        """The checks the two k-means calls share: vec (N, C) and cen (K, C) fp32, K <= N, both 16-byte aligned (the kernels read
        them 16 bytes at a time: a view that starts at an odd element is refused), and `others` = [(what, tensor, dtype,
        shape)], all contiguous on vec's device -> (N, C, K)."""
        def ok(t, dtype, shape=None):
            return isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_cuda and t.is_contiguous() and \
                (shape is None or tuple(t.shape) == shape) and (t is vec or t.device == vec.device)

        if not (ok(vec, torch.float32) and vec.dim() == 2 and 1 <= vec.shape[0] < 2 ** 31 and 4 <= vec.shape[1] <= 1024 and
                vec.shape[1] % 4 == 0 and vec.data_ptr() % 16 == 0):
            raise ValueError(f"{name}: vec must be a contiguous, 16-byte aligned (N, C) fp32 device tensor, 1 <= N < 2^31, C a multiple "
                             f"of 4 in 4..1024")
        N, C = int(vec.shape[0]), int(vec.shape[1])
        if not (ok(cen, torch.float32) and cen.dim() == 2 and int(cen.shape[1]) == C and 1 <= cen.shape[0] <= N and
                cen.data_ptr() % 16 == 0):
            raise ValueError(f"{name}: cen must be a contiguous, 16-byte aligned (K, C = {C}) fp32 tensor on vec's device with "
                             f"1 <= K <= N = {N}")
        K = int(cen.shape[0])
        for what, t, dtype, shape in others:
            shape = tuple(K if n == "K" else N if n == "N" else n for n in shape)
            if not ok(t, dtype, shape):
                raise ValueError(f"{name}: {what} must be a contiguous {shape} {str(dtype)[6:]} tensor on vec's device")
        return N, C, K

    def units_kmeans_assign_(self, vec, cen, cnrm, assign, moved):
        """The assignment step of the index reduction (`ddsp_units_kmeans_assign`; include/ddsp_amd.h states the rule): every
        entry of vec (N, C) fp32 goes to the centre of cen (K, C) with the smallest (cnrm[j] - 2 <x, cen[j]>, j), cnrm (K,) fp32
        the centres' norms (`units_index_norms`).  In place: assign (N,) int32 is read as the previous assignment and
        overwritten, moved (1,) int32 grows by the number of entries that changed.  -> assign."""
        N, C, K = self._kmeans_shapes("units_kmeans_assign_", vec, cen, [("cnrm", cnrm, torch.float32, ("K",)),
                                                                          ("assign", assign, torch.int32, ("N",)),
                                                                          ("moved", moved, torch.int32, (1,))])
        self.call("ddsp_units_kmeans_assign", _ptr(vec), N, C, _ptr(cen), _ptr(cnrm), K, _ptr(assign), _ptr(moved))
        return assign

    def units_kmeans_update_(self, vec, assign, cen, count, shift, workspace):
        """The update step of the index reduction (`ddsp_units_kmeans_update`): in place, centre j of cen (K, C) fp32 becomes the
        mean of the entries of vec (N, C) with assign (N,) int32 == j, formed exactly in 64-bit fixed point at `shift` (an int:
        62 - E - L of the rule, from the host); a centre without entries keeps its bits, an assignment outside [0, K) belongs to
        no centre.  count (K,) int32 receives the entries of every centre; workspace: at least K * C * 8 bytes on vec's device,
        any dtype, zeroed by the call.  -> cen."""
        N, C, K = self._kmeans_shapes("units_kmeans_update_", vec, cen, [("assign", assign, torch.int32, ("N",)),
                                                                          ("count", count, torch.int32, ("K",))])
        if isinstance(shift, bool) or not isinstance(shift, int) or not -97 <= shift <= 210:
            raise ValueError(f"units_kmeans_update_: shift must be an int in -97..210 (62 - E - L of the rule), got {shift!r}")
        if not (isinstance(workspace, torch.Tensor) and workspace.is_cuda and workspace.device == vec.device and
                workspace.is_contiguous() and workspace.numel() * workspace.element_size() >= K * C * 8 and
                workspace.data_ptr() % 16 == 0):
            raise ValueError(f"units_kmeans_update_: workspace must be a contiguous, 16-byte aligned tensor of at least K * C * 8 = "
                             f"{K * C * 8} bytes on vec's device")
        self.call("ddsp_units_kmeans_update", _ptr(vec), N, C, _ptr(assign), K, shift, _ptr(cen), _ptr(count), _ptr(workspace),
                  int(workspace.numel()) * workspace.element_size())
        return cen

    def bank_features_gather_(self, rows, units, f0, volume, mix, cunits, cf0, cvolume, cmix, noise=None, cnoise=None):
        """The rows of one model out of a call's row batch (`ddsp_bank_features_gather`): rows (W,) int32 device, entry r the row
        of the batch behind compact row r, -1 (or anything outside [0, R)) for padding.  In place: cunits (W, Fr, C), cf0 (W, Fr, 1)
        or (W, Fr), cvolume (W, Fr), cmix = (ids (W, K) int32, w (W, K)) and cnoise (W, T) take the named rows of units (R, Fr, C),
        f0, volume, mix and noise (R, T) (noise and cnoise both None: no injected noise).  A padding row gets zeros and speaker 1
        with weight 1.  -> cunits."""
        W, (R, Fr, C) = rows.numel(), units.shape
        K = check_mix_rows(mix[0], mix[1], R)
        floats = [units, f0, volume, cunits, cf0, cvolume] + ([] if noise is None else [noise, cnoise])
        if (noise is None) != (cnoise is None) or rows.dtype != torch.int32 or rows.dim() != 1 or check_mix_rows(*cmix, W) != K or \
                any(t.dtype != torch.float32 or not t.is_contiguous() for t in floats):
            raise ValueError("bank_features_gather_: contiguous fp32 tensors, a (W,) int32 row table and mix tables of one K")
        sizes = ((cunits, W, Fr * C), (f0, R, Fr), (cf0, W, Fr), (volume, R, Fr), (cvolume, W, Fr))   # (f0 may carry a last 1)
        if any(t.shape[0] != n or t.numel() != n * m for t, n, m in sizes):
            raise ValueError("bank_features_gather_: R rows of the batch (units (R, Fr, C), f0, volume (R, Fr)) and W compact rows")
        T = 1
        if noise is not None:
            T = noise.shape[-1]
            if tuple(noise.shape) != (R, T) or tuple(cnoise.shape) != (W, T):
                raise ValueError("bank_features_gather_: noise (R, T) and cnoise (W, T)")
        self.call("ddsp_bank_features_gather", _ptr(rows), W, R, Fr, C, T, _ptr(units), _ptr(f0), _ptr(volume), _ptr(noise),
                  _ptr(mix[0]), _ptr(mix[1]), K, _ptr(cunits), _ptr(cf0), _ptr(cvolume), _ptr(cnoise), _ptr(cmix[0]), _ptr(cmix[1]))
        return cunits

    def bank_signal_scatter_(self, rows, csig, sig):
        """The gated signal of one model's compact rows into the call's signal (`ddsp_bank_signal_scatter`): sig (R, T)[rows[r]] =
        csig (W, T)[r] for every row of rows (W,) int32 that is no padding; the other rows of sig stay.  -> sig."""
        W, T = csig.shape
        if rows.dtype != torch.int32 or tuple(rows.shape) != (W,) or sig.dim() != 2 or sig.shape[1] != T:
            raise ValueError("bank_signal_scatter_: csig (W, T), sig (R, T) and a (W,) int32 row table")
        if csig.dtype != torch.float32 or sig.dtype != torch.float32 or not (csig.is_contiguous() and sig.is_contiguous()):
            raise ValueError("bank_signal_scatter_: the signals must be contiguous fp32")
        self.call("ddsp_bank_signal_scatter", _ptr(rows), W, sig.shape[0], _ptr(csig), T, _ptr(sig))
        return sig

    def phase_vocoder(self, a, b, fade_out, fade_in):
        """gui.py:14-31: cross-fade of the kept tail `a` into the new head `b` (both (n,)) with a phase-interpolated
        oscillator term; returns (n,)."""
        a, b = a.contiguous().float(), b.contiguous().float()
        fo, fi = fade_out.contiguous().float(), fade_in.contiguous().float()
        if a.dim() == 2:   # S streams: a, b (S, n) with the shared fade windows (n,) -> (S, n), every row like the solo call
            S, n = a.shape
            if tuple(b.shape) != (S, n) or not (fo.numel() == fi.numel() == n):
                raise ValueError("phase_vocoder: a and b must be (S, n) and the fade windows (n,)")
        else:
            S, n = 1, a.numel()
            if not (b.numel() == fo.numel() == fi.numel() == n):
                raise ValueError("phase_vocoder: a, b and the fade windows must have the same length")
        out = torch.empty((S, n) if a.dim() == 2 else (n,), device=a.device, dtype=torch.float32)
        self.call("ddsp_phase_vocoder", _ptr(a), _ptr(b), _ptr(fo), _ptr(fi), S, n, _ptr(out))
        return out

    # -- a15 -----------------------------------------------------------------------------------
    def volume_gate_(self, signal, volume, threshold_db, hop):
        """In place: signal (B,T) *= upsample(dilate9(volume > 10^(dB/20)))."""
        B, T = signal.shape
        vol = volume.reshape(B, -1).contiguous().float()
        self.call("ddsp_volume_gate", _ptr(signal), _ptr(vol), float(10 ** (float(threshold_db) / 20)), B,
                  vol.shape[1], int(hop))
        return signal

    def volume_gate_rows_(self, signal, volume, start_dev, n_dev, threshold_db, hop, file_dev=None, file_frames_dev=None):
        """In place, for a ragged batch of slices of ONE file: signal (B, T_max) fp32, row b's samples t < n[b] * hop times the
        file's gate (`volume_gate_` of the whole `volume` (Fr,)) at start[b] * hop + t; the rest of a row is not touched.
        start_dev, n_dev: (B,) int32 device tensors (`ragged_counts`).  One launch (`ddsp_volume_gate_rows`), nothing is read
        back: a row outside the file's frames or its own row stays as it is and raises ValueError from `poll_error()` after a
        synchronise or from the next call that takes the error word.
        file_dev (B,) and file_frames_dev (F,) int32 device tensors, both or neither: the rows are slices of SEVERAL files,
        `volume` is (F, Fr_max) fp32 contiguous and row b is gated by the track of file[b], which ends at that file's own frame
        count (`ddsp_volume_gate_files`): each row as the one-file call on its file alone gates it."""
        if signal.dim() != 2 or signal.dtype != torch.float32 or not signal.is_contiguous():
            raise ValueError("volume_gate_rows_: signal must be a contiguous fp32 (B, T_max) tensor (it is gated in place)")
        if (file_dev is None) != (file_frames_dev is None):
            raise ValueError("volume_gate_rows_: file_dev and file_frames_dev come together or not at all")
        B, T_max = signal.shape
        thr = float(10 ** (float(threshold_db) / 20))
        if file_dev is None:
            vol = volume.reshape(-1).contiguous().float()
            symbol, head, Fr = "ddsp_volume_gate_rows", (), vol.numel()
        else:
            if volume.dim() != 2 or volume.dtype != torch.float32 or not volume.is_contiguous():
                raise ValueError("volume_gate_rows_: with file_dev, volume must be a contiguous fp32 (F, Fr_max) tensor")
            vol, (F, Fr) = volume, volume.shape
            symbol, head = "ddsp_volume_gate_files", (_ptr(self._counts_dev(file_frames_dev, F)), F, _ptr(self._counts_dev(file_dev, B)))
        if B:
            self.call(symbol, _ptr(signal), _ptr(vol), *head, _ptr(self._counts_dev(start_dev, B)),
                      _ptr(self._counts_dev(n_dev, B)), thr, B, T_max, Fr, int(hop))
        return signal

    # -- the rows of a ragged group from several files -------------------------------------------
    def pieces_gather(self, table_dev, n_file_samples_dev, n_file_frames_dev, audio=None, S_max=0, f0=None, volume=None,
                      key_factor=None, N_max=0, key_timeline=None):
        """One launch (`ddsp_pieces_gather`) forms the R rows of a ragged group from a padded batch of F files.  table_dev
        (R, 5) int32 device rows (file, start_frame, n_frames, start_sample, n_samples); n_file_samples_dev / n_file_frames_dev
        (F,) int32 device.  audio (F, T_max) with S_max -> wav (R, S_max); f0, volume (F, Fr_max) and key_factor (F,) with N_max
        -> f0_rows (the one rounded product f0 * key_factor[file]) and vol_rows (R, N_max; not made when `volume` is None);
        exact zeros behind every piece.
        A table of (R, 6) rows holds the rows of JOBS (`ddsp_pieces_gather_jobs`): the sixth column is the row's job, the file
        still names the source, and key_factor is (J,), one per job - J jobs over one file read that file's features in place.
        key_timeline=(bp_off (J + 1,) int32, bp_frame (P,) int32, bp_semi (P,) fp32, bp_fac (P,) fp32), contiguous device tensors,
        in place of `key_factor` (which stays None) with a table of (R, 6) rows: the jobs' keys move over their files
        (`ddsp_pieces_gather_keys`).  Job j owns the breakpoints bp_off[j] .. bp_off[j + 1] - 1, in file frames; f0_rows is f0
        times the factor at every frame's own file frame (include/ddsp_amd.h states the rule), a job with one breakpoint the
        bits of `key_factor`.  A job whose range is empty or leaves [0, P) gives a row of zeros and the error word.
        Returns (wav, f0_rows, vol_rows), None for the half that was not asked for.  Nothing is read back: a piece outside its
        file gives a row of zeros and raises ValueError from `poll_error()` after a synchronise or from the next call that takes
        the error word."""
        def dense(name, t, shape):
            if not (isinstance(t, torch.Tensor) and t.device == self.device and t.dtype == torch.float32 and t.is_contiguous()
                    and (shape is None or tuple(t.shape) == shape)):
                raise ValueError(f"pieces_gather: {name} must be a contiguous fp32 tensor on {self.device}"
                                 + (f" of shape {shape}" if shape else ""))
            return t
        if table_dev.dim() != 2 or table_dev.shape[1] not in (5, 6) or table_dev.dtype != torch.int32 or not table_dev.is_cuda \
                or not table_dev.is_contiguous():
            raise ValueError("pieces_gather: the table must be a contiguous (R, 5) int32 device tensor ((R, 6): rows of jobs)")
        by_job = table_dev.shape[1] == 6
        if key_timeline is not None:
            if not by_job or key_factor is not None or not (isinstance(key_timeline, (tuple, list)) and len(key_timeline) == 4):
                raise ValueError("pieces_gather: key_timeline=(bp_off, bp_frame, bp_semi, bp_fac) goes with a table of (R, 6) rows "
                                 "and without key_factor")
            bp_off, bp_frame, bp_semi, bp_fac = key_timeline
            P = bp_frame.numel() if isinstance(bp_frame, torch.Tensor) else 0
            for t, dtype in ((bp_off, torch.int32), (bp_frame, torch.int32), (bp_semi, torch.float32), (bp_fac, torch.float32)):
                if not (isinstance(t, torch.Tensor) and t.device == self.device and t.dtype == dtype and t.dim() == 1 and
                        t.is_contiguous()):
                    raise ValueError(f"pieces_gather: key_timeline holds contiguous 1-d tensors on {self.device}: bp_off, bp_frame "
                                     "int32, bp_semi, bp_fac fp32")
            if bp_off.numel() < 2 or P < 1 or bp_semi.numel() != P or bp_fac.numel() != P:
                raise ValueError("pieces_gather: key_timeline: bp_off (J + 1,) with J >= 1 and bp_frame, bp_semi, bp_fac (P,) with "
                                 "P >= 1")
        if audio is None and f0 is None:
            raise ValueError("pieces_gather: pass audio, or f0 with key_factor (and volume), or both")
        R, F = table_dev.shape[0], n_file_samples_dev.numel()
        self._counts_dev(n_file_samples_dev, F)
        self._counts_dev(n_file_frames_dev, F)
        wav = f0_rows = vol_rows = None
        T_max = Fr_max = 1
        if audio is not None:
            T_max = dense("audio", audio, None).shape[1] if audio.dim() == 2 and audio.shape[0] == F else -1
            wav = torch.empty(R, int(S_max), device=self.device, dtype=torch.float32)
        if f0 is not None:
            Fr_max = dense("f0", f0, None).shape[1] if f0.dim() == 2 and f0.shape[0] == F else -1
            if key_timeline is None:
                dense("key_factor", key_factor, (key_factor.numel(),) if by_job and isinstance(key_factor, torch.Tensor) else (F,))
            f0_rows = torch.empty(R, int(N_max), device=self.device, dtype=torch.float32)
            if volume is not None:
                dense("volume", volume, (F, Fr_max))
                vol_rows = torch.empty(R, int(N_max), device=self.device, dtype=torch.float32)
        elif volume is not None:
            raise ValueError("pieces_gather: volume goes with f0")
        if T_max < 1 or Fr_max < 1:
            raise ValueError(f"pieces_gather: audio must be (F, T_max) and f0 (F, Fr_max) with F = {F} files and at least a column")
        # (a table of jobs with the sample half alone has no key factors: J = 1 lets only job 0 pass, and nothing reads it)
        symbol, jobs = ("ddsp_pieces_gather_jobs", (1 if key_factor is None else key_factor.numel(),)) if by_job else \
            ("ddsp_pieces_gather", ())
        key = (_ptr(key_factor),)
        if key_timeline is not None:
            symbol, jobs = "ddsp_pieces_gather_keys", (bp_off.numel() - 1,)
            key = (_ptr(bp_off), _ptr(bp_frame), _ptr(bp_semi), _ptr(bp_fac), P)
        if R:
            self.call(symbol, _ptr(audio), _ptr(f0), _ptr(volume), *key, _ptr(n_file_samples_dev), _ptr(n_file_frames_dev), F, T_max,
                      Fr_max, *jobs, _ptr(table_dev), R, int(S_max), int(N_max), _ptr(wav), _ptr(f0_rows), _ptr(vol_rows))
        return wav, f0_rows, vol_rows

    # -- the stitch ----------------------------------------------------------------------------
    def stitch(self, pieces, p, fade, total):
        """pieces: S fp32 device tensors (views into ragged group tensors included; the samples of one piece contiguous);
        p, fade: their first output sample and cross-faded length (`infer_offline.stitch_plan`, which has checked them);
        -> the fp64 device tensor (total,) of `ddsp_stitch`: one table upload, one launch, no copy per piece."""
        if not (len(pieces) == len(p) == len(fade)):
            raise ValueError(f"stitch: {len(pieces)} pieces, {len(p)} positions and {len(fade)} fades")
        rows = []
        for i, (x, pi, fi) in enumerate(zip(pieces, p, fade)):
            if x.dtype != torch.float32 or x.device != self.device or not x.is_contiguous():
                raise ValueError(f"stitch: piece {i} must be fp32 on {self.device} with its samples contiguous")
            rows.append((x.data_ptr(), int(pi), x.numel(), int(fi)))
        out = torch.empty(int(total), device=self.device, dtype=torch.float64)
        if int(total):
            table = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4).to(self.device)
            self.call("ddsp_stitch", _ptr(table), len(rows), _ptr(out), int(total))
        return out

    def pcm16(self, x, spans=None):
        """x: a contiguous fp64 device waveform (n,) (a view from any element of a larger tensor is fine); spans: None - the one
        span (0, n) - or [(base, total)] ascending and disjoint with even bases, as `infer_offline.stitch_plan_many` lays files
        out (ValueError otherwise, before anything is launched) -> (int16 device tensor (n,), peak (J,) fp64 device, clipped
        (J,) int64 device) from one `ddsp_pcm16` launch: `clip(rint(x * 32768), -32768, 32767)` bit for bit as numpy computes it
        on the host (`main.pcm16`), exact zeros between the spans, and per span the largest |x| and the number of clipped
        samples.  2 bytes per sample to read back in place of 8.  Nothing is read back here."""
        if not (isinstance(x, torch.Tensor) and x.dim() == 1 and x.dtype == torch.float64 and x.device == self.device
                and x.is_contiguous()):
            raise ValueError(f"pcm16: x must be a contiguous fp64 (n,) tensor on {self.device}")
        n = x.numel()
        table, J = None, 1
        if spans is not None:
            rows, end = [(int(base), int(total)) for base, total in spans], 0
            for j, (base, total) in enumerate(rows):
                if base < end or base % 2 or total < 0 or base + total > n:
                    raise ValueError(f"pcm16: span {j} ({base}, {total}) must start at an even sample at or behind the end of the "
                                     f"span before it ({end}) and end inside the {n} samples")
                end = base + total
            J = len(rows)
            table = torch.tensor(rows, dtype=torch.int64).reshape(-1, 2).to(self.device)
        peak = torch.zeros(J, device=self.device, dtype=torch.float64)
        clipped = torch.zeros(J, device=self.device, dtype=torch.int64)
        if J == 0:                       # no span covers anything (an empty table has no address to pass)
            return torch.zeros(n, device=self.device, dtype=torch.int16), peak, clipped
        out = torch.empty(n, device=self.device, dtype=torch.int16)
        if n:
            self.call("ddsp_pcm16", _ptr(x), n, _ptr(table), J, _ptr(out), _ptr(peak), _ptr(clipped))
        return out, peak, clipped


class ResamplePlan:
    """The handle of `Context.resample_plan`: frees the plan's tables with the object (a device synchronisation)."""

    def __init__(self, lib, handle, pairs, lowpass_filter_width, device):
        self.lib, self.handle, self.pairs, self.lowpass_filter_width, self.device = lib, handle, pairs, lowpass_filter_width, device

    def length(self, T):
        """Padded output width for inputs of width T: the largest `ddsp_resample_length` over the pairs."""
        return int(self.lib.ddsp_resample_keyed_length(self.handle, int(T)))

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.ddsp_resample_keyed_plan_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def key_thresholds(max_key=12):
    """thr[k], k = 0..max_key: the largest fp32 value <= 2^(k/12), from fp64 (a host computation) -> float32 numpy array.  An
    fp32 quotient q has ceil(12 log2 q) <= k exactly when q <= thr[k]: 2^(k/12) is irrational except at k = 0 and 12, where it
    is an fp32 value itself, so no fp32 q lies close enough to it for the fp64 rounding of numpy's log2 to matter."""
    import numpy as np
    thr = np.empty(int(max_key) + 1, dtype=np.float32)
    for k in range(int(max_key) + 1):
        exact = 2.0 ** (k / 12.0)
        t = np.float32(exact)
        thr[k] = t if float(t) <= exact else np.nextafter(t, np.float32(0))
    return thr


def key_from_thresholds(f0_max, thr):
    """The host form of `ddsp_enhancer_keys`' 'auto' rule for one f0 maximum (what the kernel computes; tests hold it against
    the reference's numpy expression)."""
    import numpy as np
    m = np.float32(f0_max)
    if not m > 0:
        return 0
    q = m / np.float32(760)
    for k in range(len(thr)):
        if q <= thr[k]:
            return k
    return len(thr) - 1


_contexts = {}
_ctx_lock = threading.Lock()


_override = threading.local()


def next_dither_seed(seed):
    """The value `ddsp_crepe_decode` leaves in its `seed_dev` word after a call that read `seed` (a host computation)."""
    return (int(seed) * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)


def seed_from_torch():
    """A seed for an in-kernel generator, drawn from torch's default generator (so `torch.manual_seed` repeats a run)."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def resample_length(n, sr_in, sr_out):
    """n samples at `sr_in` as samples at `sr_out`: n itself at equal rates, else the resampler's length
    (`ddsp_resample_length`; negative for a pair of rates it cannot convert)."""
    return n if int(sr_in) == int(sr_out) else int(load_library().ddsp_resample_length(int(n), int(sr_in), int(sr_out)))


def hubert_base_frames(T):
    """Frames of T samples in the base-form units encoder, which does not pad (`ddsp_hubert_base_frames`): 0 when too short."""
    return int(load_library().ddsp_hubert_base_frames(int(T)))


def hubert_frames(T):
    """Encoder frames of T samples (`ddsp_hubert_frames`, a host computation): 0 when the audio is too short."""
    return int(load_library().ddsp_hubert_frames(int(T)))


def crepe_frames(T16, hop=80):
    """CREPE frames of T16 samples at 16 kHz with pad=True (`ddsp_crepe_frames`, a host computation): 1 + T16 // hop."""
    n = int(load_library().ddsp_crepe_frames(int(T16), int(hop)))
    if n < 0:
        raise ValueError(f"crepe_frames: bad length {T16} or hop {hop}")
    return n


def f0_ac_frames(T, sr, hop, f0_min):
    """Analysis frames of T samples for the autocorrelation f0 extractor (`ddsp_f0_ac_frames`, a host computation): 0 when the
    audio is shorter than one window of 3 / f0_min seconds."""
    n = int(load_library().ddsp_f0_ac_frames(int(T), int(sr), float(hop), float(f0_min)))
    if n < 0:
        raise ValueError(f"f0_ac_frames: bad length {T}, rate {sr}, hop {hop} or f0_min {f0_min}")
    return n


def slicer_frames(n, win, hop):
    """RMS frames of n samples for the silence slicer (`ddsp_slicer_frames`, a host computation):
    1 + (n + 2 * (win // 2) - win) // hop."""
    F = int(load_library().ddsp_slicer_frames(int(n), int(win), int(hop)))
    if F < 0:
        raise ValueError(f"slicer_frames: bad length {n}, window {win} or hop {hop}")
    return F


def slicer_capacity(F_max, min_interval):
    """Rows of the slicer's chunk table that always suffice for rows of at most F_max frames (include/ddsp_amd.h): at most
    F_max // min_interval tags with a silent run of their own, one more by the leading rule, and 2 K + 1 chunks for K tags."""
    if int(min_interval) < 1 or int(F_max) < 0:
        raise ValueError(f"slicer_capacity: bad frame count {F_max} or min_interval {min_interval} (frames)")
    return 2 * (int(F_max) // int(min_interval) + 1) + 1


def crepe_ragged_table(n16, hop=80):
    """Checked per-row 16 kHz sample counts -> the list of 2B + 1 ints a ragged `crepe_activations` uploads once: the B
    counts, then the B + 1 exclusive prefix sums of the rows' frame counts (the packed frame list; its last entry is the
    number of frames the network runs over)."""
    prefix = [0]
    for v in n16:
        prefix.append(prefix[-1] + crepe_frames(v, hop))
    return list(n16) + prefix


class use_context:
    """`with use_context(ctx):` makes `context_for` return `ctx` on this thread for that device - how a graph-capturing
    caller routes a model's library calls through a context of its own (graphed.GraphedSynth)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.prev = getattr(_override, "ctx", None)
        _override.ctx = self.ctx
        return self.ctx

    def __exit__(self, *exc):
        _override.ctx = self.prev
        return False


def context_for(device):
    """Per (device, thread) context cache (one handle per stream/thread)."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else (torch.cuda.current_device() if torch.cuda.is_available() else 0)
    forced = getattr(_override, "ctx", None)
    if forced is not None and dev.type == "cuda" and forced.device.index == idx:
        return forced
    key = (dev.type, idx, threading.get_ident())
    with _ctx_lock:
        ctx = _contexts.get(key)
        if ctx is None:
            ctx = Context(torch.device(dev.type, idx) if dev.type == "cuda" else dev)
            _contexts[key] = ctx
    return ctx
