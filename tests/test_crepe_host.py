"""CPU-side checks of the CREPE f0 extractor surface: the state-dict contract of ddsp.crepe.Crepe ('full' and 'tiny'), the
frame count, bins <-> Hz and the range mask, the restated post-filter against the reference's own (tests/golden/
ref_crepe_postfilter.npz), the exact banded Viterbi form against the full-matrix decode, and the refusals."""
import os

import numpy as np
import pytest
import torch

import crepe_cases as CC
from conftest import GOLDEN

FIX = os.path.join(GOLDEN, "ref_crepe_postfilter.npz")


@pytest.fixture(scope="module")
def fix():
    return np.load(FIX)


@pytest.mark.parametrize("model", ["full", "tiny"])
def test_state_dict_keys_and_shapes(model):
    from ddsp.crepe import Crepe
    sd = Crepe(model).state_dict()
    want = CC.state_dict_shapes(model)
    assert list(sd) == list(want)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert len(sd) == 6 * 7 + 2
    # the deterministic fill loads strictly
    Crepe(model).load_state_dict(CC.fill(model), strict=True)


def test_weight_struct_is_the_header_layout():
    import ctypes
    import hipddsp
    assert ctypes.sizeof(hipddsp.CrepeWeights) == 8 * 38 + 4 * 6 + 8
    assert hipddsp.CrepeWeights.version.offset == 8 * 38 + 4 * 6
    assert hipddsp.ABI_VERSION == 8


def test_frame_count(lib_path):
    import hipddsp
    for T in (0, 1, 79, 80, 81, 159, 160, 7777, 16000, 48595):
        assert hipddsp.crepe_frames(T) == 1 + T // 80
    assert hipddsp.crepe_frames(1000, 100) == 11
    with pytest.raises(ValueError):
        hipddsp.crepe_frames(-1)


def test_bins_and_range_mask():
    from ddsp import crepe
    # torchcrepe.convert: bin 0 is 10 * 2^(1997.38 / 1200) Hz ~ 31.7 Hz, 20 cents per bin
    assert abs(float(crepe.bin_to_frequency(0)) - 10 * 2 ** (CC.CENTS_OFFSET / 1200)) < 1e-4
    hz = crepe.bin_to_frequency(torch.arange(360))
    ratio = (hz[1:] / hz[:-1]).double()
    assert torch.allclose(ratio, torch.full_like(ratio, 2 ** (20 / 1200)), rtol=1e-6)
    for f in (31.0, 50.0, 65, 100.0, 800, 1100.0, 2006.0):
        assert crepe.frequency_to_bin(f) == CC.frequency_to_bin(f)
        assert crepe.frequency_to_bin(f, ceil=True) == CC.frequency_to_bin(f, ceil=True)
    assert CC.mask_range(65, 800) == (62, 280)
    assert CC.mask_range(20, 4000) == (320, 360)   # minidx = -40: a negative minidx is a Python slice from the end


def test_postfilter_restatement_matches_the_reference(fix):
    for i in range(len(fix["sr"])):
        got = CC.postfilter(fix[f"f0_in_{i}"], fix[f"pd_in_{i}"], int(fix["sr"][i]), float(fix["hop"][i]), int(fix["n_frames"][i]),
                            int(fix["start_frame"][i]), bool(fix["uv_interp"][i]), float(fix["f0_min"][i]))
        want = fix[f"out_{i}"]
        assert got.dtype == np.float32 and got.shape == want.shape
        ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, (i, int(ulp.max()))


def test_bookkeeping_and_16k_length_match_the_reference(fix, lib_path):
    """n_frames, start_frame, the crop and the 16 kHz length F0_Extractor.extract computes for the reference's cases."""
    import hipddsp
    lib = hipddsp.load_library()
    for i in range(len(fix["sr"])):
        sr, hop, T, sf = int(fix["sr"][i]), float(fix["hop"][i]), int(fix["T"][i]), float(fix["silence_front"][i])
        n_frames, start_frame, crop = CC.extract_bookkeeping(T, sr, hop, sf)
        assert (n_frames, start_frame) == (int(fix["n_frames"][i]), int(fix["start_frame"][i]))
        T16 = int(lib.ddsp_resample_length(T - crop, sr, 16000)) if sr != 16000 else T - crop
        assert T16 == int(fix["T16"][i]), (i, T16, int(fix["T16"][i]))


def test_banded_viterbi_equals_the_full_matrix_decode():
    rng = np.random.default_rng(5)
    # random emissions, and tracks whose best path jumps out of the +-11-bin band (cost log(tiny) ~ -87.3 per jump)
    cases = [CC.emissions(rng.uniform(0, 1, (40, 360)), 50, 1100)]
    path = CC.known_path()
    cases.append(CC.emissions(CC.bump_track(len(path), path), 50, 1100))
    noisy = CC.bump_track(len(path), path) + rng.uniform(0, 0.05, (len(path), 360)).astype(np.float32)
    cases.append(CC.emissions(noisy, 50, 1100))
    for k, e in enumerate(cases):
        naive, _ = CC.viterbi_naive(e)
        assert np.array_equal(CC.viterbi_banded(e), naive), k
    np.testing.assert_array_equal(CC.viterbi_naive(cases[1])[0], path)
    np.testing.assert_array_equal(CC.viterbi_naive(cases[2])[0], path)
    # states far from the best one (here: the masked bins) take their best predecessor from outside the band: a decode
    # restricted to the band would differ there
    assert CC.out_of_band_choices(cases[2]) > 1000


def test_cpu_only_extractors_raise():
    from ddsp.vocoder import F0_Extractor
    for name in ("parselmouth", "dio", "harvest"):
        with pytest.raises(NotImplementedError, match="crepe"):
            F0_Extractor(name, 44100, 512)
    with pytest.raises(ValueError):
        F0_Extractor("no-such-extractor", 44100, 512)


def test_missing_checkpoint_says_how_to_pass_one():
    import importlib.util
    from ddsp.vocoder import _find_torchcrepe_checkpoint
    if importlib.util.find_spec("torchcrepe") is None:
        with pytest.raises(FileNotFoundError, match="crepe_ckpt"):
            _find_torchcrepe_checkpoint()
    else:
        try:
            assert os.path.isfile(_find_torchcrepe_checkpoint())
        except FileNotFoundError as e:
            assert "crepe_ckpt" in str(e)


def test_cpu_tensor_raises():
    from ddsp.crepe import Crepe
    with pytest.raises(RuntimeError):
        Crepe("tiny").activations(torch.zeros(1, 1600))


def test_restated_network_shapes_and_range():
    sd = CC.fill("tiny")
    p = CC.activations64(sd, CC.audio("odd")[:, :1600])
    assert p.shape == (1, 1 + 1600 // 80, 360)
    assert float(p.min()) > 0 and float(p.max()) < 1
