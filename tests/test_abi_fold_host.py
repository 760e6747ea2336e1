"""One C entry point per operation (ABI 8), host side (no GPU): the header declares no twin, the library exports none of the
folded names, every binding method of a folded operation names one symbol, and the version pins agree."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

SUFFIXES = ("_ragged", "_batch", "_scaled", "_dseed", "_share")

# the names ABI 8 folded into their un-suffixed twin (ddsp_stft_frames_ragged: renamed to ddsp_stft_frames)
REMOVED = [
    "ddsp_unit2ctrl_fwd_ragged", "ddsp_unit2ctrl_fwd_rowmix_ragged", "ddsp_unit2ctrl_bwd_ragged", "ddsp_unit2ctrl_fwd_keep_ragged",
    "ddsp_unit2ctrl_bwd_kept_ragged", "ddsp_rss_loss_ragged", "ddsp_rss_loss_share", "ddsp_adamw_step_multi_scaled",
    "ddsp_volume_extract_ragged", "ddsp_align_units_ragged", "ddsp_retime_f0_ragged", "ddsp_resample_ragged", "ddsp_conv1d_ragged",
    "ddsp_conv1d_pair_ragged", "ddsp_nsf_post_ragged", "ddsp_nsf_source_ragged", "ddsp_nsf_noise_conv_ragged",
    "ddsp_stft_frames_ragged", "ddsp_softmax_attention_ragged", "ddsp_hubert_soft_units_ragged", "ddsp_hubert_encode_ragged",
    "ddsp_crepe_activations_ragged", "ddsp_crepe_decode_ragged", "ddsp_crepe_decode_dseed", "ddsp_f0_postfilter_ragged",
    "ddsp_f0_ac_ragged", "ddsp_slicer_ragged", "ddsp_stream_push_batch", "ddsp_sola_batch", "ddsp_phase_vocoder_batch"]

# binding method -> the symbols it may name: one per operation (`retime_f0` and `rss_loss` also serve ddsp_retime_f0_keyed and
# ddsp_rss_loss_rows, `volume_extract` ddsp_volume_extract_frac: operations of their own that were never twins)
METHODS = {
    "unit2ctrl": {"ddsp_unit2ctrl_fwd", "ddsp_unit2ctrl_fwd_rowmix"}, "unit2ctrl_bwd": {"ddsp_unit2ctrl_bwd"},
    "unit2ctrl_keep": {"ddsp_unit2ctrl_fwd_keep", "ddsp_unit2ctrl_keep_bytes"}, "unit2ctrl_bwd_kept": {"ddsp_unit2ctrl_bwd_kept"},
    "rss_loss": {"ddsp_rss_loss", "ddsp_rss_loss_rows"}, "adamw_step_multi": {"ddsp_adamw_step_multi"},
    "volume_extract": {"ddsp_volume_extract", "ddsp_volume_extract_frac"}, "align_units": {"ddsp_align_units"},
    "retime_f0": {"ddsp_retime_f0", "ddsp_retime_f0_keyed"}, "resample": {"ddsp_resample", "ddsp_resample_length"},
    "conv1d": {"ddsp_conv1d"}, "conv1d_pair": {"ddsp_conv1d_pair"}, "nsf_post": {"ddsp_nsf_post"}, "nsf_source": {"ddsp_nsf_source"},
    "nsf_noise_conv": {"ddsp_nsf_noise_conv"}, "stft_frames": {"ddsp_stft_frames"}, "softmax_attention": {"ddsp_softmax_attention"},
    "hubert_units": {"ddsp_hubert_soft_units"}, "hubert_encode": {"ddsp_hubert_encode"},
    "crepe_activations": {"ddsp_crepe_activations"}, "crepe_decode": {"ddsp_crepe_decode"}, "f0_postfilter": {"ddsp_f0_postfilter"},
    "f0_ac": {"ddsp_f0_ac"}, "slicer": {"ddsp_slicer"}, "stream_push_": {"ddsp_stream_push"}, "sola": {"ddsp_sola"},
    "phase_vocoder": {"ddsp_phase_vocoder"}}


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddsp_amd.h")).read(), flags=re.S)
    return re.findall(r"\b(ddsp_\w+)\s*\(", text)


def test_header_declares_no_twin():
    names = _declared()
    assert len(names) > 80
    assert not [n for n in names if n.endswith(SUFFIXES)]
    assert not set(names) & set(REMOVED)


def test_library_exports_no_folded_name(lib_path):
    import hipddsp
    lib = ctypes.CDLL(lib_path)
    assert hasattr(lib, "ddsp_stft_frames") and hasattr(lib, "ddsp_rss_loss_rows")     # (hasattr does find what is exported)
    assert not [n for n in REMOVED if hasattr(lib, n)]
    assert not [n for n in hipddsp.SIGNATURES if n in REMOVED or n.endswith(SUFFIXES)]


def test_binding_methods_name_one_symbol_per_operation():
    import hipddsp
    for method, allowed in METHODS.items():
        src = inspect.getsource(getattr(hipddsp.Context, method))
        called = set(re.findall(r"call\(\s*\"(ddsp_\w+)\"", src))
        assert called and called <= allowed, (method, called)
        mentioned = set(re.findall(r"\bddsp_\w+", src)) - {"ddsp_amd"}
        assert mentioned <= allowed, (method, mentioned)
        # an operation is called from one place: no fork between two forms of it
        for name in called:
            assert len(re.findall(r"call\(\s*\"%s\"" % name, src)) == 1, (method, name)


def test_abi_version_is_8_everywhere(lib_path):
    import hipddsp
    with open(os.path.join(ROOT, "ddsp-svc-official_amd", "csrc", "ctx.hip")) as fh:
        src = int(re.search(r"#define DDSP_ABI_VERSION (\d+)", fh.read()).group(1))
    assert hipddsp.ABI_VERSION == 8 == src == hipddsp.load_library().ddsp_abi_version()
