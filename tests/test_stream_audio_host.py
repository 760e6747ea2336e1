"""CPU-side checks of the raw-audio chain's surface: the new C entry points are declared, exported and bound; the host
restatement of the device seed step; the public signatures."""
import ctypes
import inspect
import os
import re

from conftest import ROOT


def test_new_entry_points_declared_exported_and_bound(lib_path):
    import hipddsp
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddsp_amd.h")).read(), flags=re.S)
    lib = ctypes.CDLL(lib_path)
    for name, n_args in (("ddsp_stream_push", 7), ("ddsp_crepe_decode", 15)):
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
        assert decl, f"{name} is not declared in include/ddsp_amd.h"
        assert len(decl.group(1).split(",")) == n_args
        assert hasattr(lib, name)
        assert len(hipddsp.SIGNATURES[name][1]) == n_args
    assert hipddsp.load_library().ddsp_abi_version() == hipddsp.ABI_VERSION


def test_next_dither_seed_is_the_64_bit_lcg_step():
    import hipddsp
    assert hipddsp.next_dither_seed(0) == 1442695040888963407
    assert hipddsp.next_dither_seed(1) == 6364136223846793005 + 1442695040888963407
    s = (1 << 64) - 1
    assert hipddsp.next_dither_seed(s) == (s * 6364136223846793005 + 1442695040888963407) % (1 << 64)
    seen, x = set(), 12345
    for _ in range(1000):
        x = hipddsp.next_dither_seed(x)
        seen.add((x >> 32, x & 0xFFFFFFFF))
    assert len({h for h, _ in seen}) == len({l for _, l in seen}) == 1000     # both halves move on every step


def test_public_signatures():
    import graphed
    import infer_offline
    import realtime
    from ddsp.vocoder import F0_Extractor
    p = inspect.signature(realtime.StreamRenderer.__init__).parameters
    assert [p[k].default for k in ("units_encoder", "f0_extractor", "f0_min", "f0_max", "f0_dither", "crepe_ckpt")] == \
        [None, None, 50, 1100, True, None]
    assert list(inspect.signature(realtime.StreamRenderer.push_audio).parameters) == ["self", "block_in", "noise", "rand_ini"]
    assert list(inspect.signature(infer_offline.convert).parameters) == [
        "model", "args", "audio", "sample_rate", "slices", "units_encoder", "f0_extractor", "spk_id", "key", "spk_mix_dict",
        "threshold_db", "enhancer", "enhancer_adaptive_key", "noise_seed"]
    assert "seed_dev" in inspect.signature(F0_Extractor.extract).parameters
    assert hasattr(graphed, "GraphedBlock") and hasattr(graphed, "block_chain")
