"""CPU-side checks of the HuBERT-Soft encoder surface: the mirror's state-dict contract against the reference's (recorded in
tests/golden/ref_hubert_soft.npz), the deterministic weight fill, the frame count, the fixture's semantics (a PyTorch
restatement of the network against the reference's fp64 output) and the no-CPU-fallback rule."""
import os

import numpy as np
import pytest
import torch

import hubert_cases as HC
from conftest import GOLDEN

FIX = os.path.join(GOLDEN, "ref_hubert_soft.npz")


@pytest.fixture(scope="module")
def fix():
    return np.load(FIX)


def _mirror_shapes():
    from ddsp.hubert import HubertSoft
    return {k: tuple(v.shape) for k, v in HubertSoft().state_dict().items()}


def test_state_dict_keys_and_shapes_match_the_reference(fix):
    shapes = _mirror_shapes()
    assert list(shapes) == list(fix["keys"])
    assert [str(s) for s in shapes.values()] == list(fix["shapes"])
    assert len(shapes) == 166


def test_weight_fill_reproduces_the_fixture_checksums(fix):
    sums = HC.checksums(HC.fill(_mirror_shapes()))
    np.testing.assert_allclose(sums, fix["checksums"], rtol=1e-12, atol=1e-9)


def test_frame_count_matches_the_reference(lib_path, fix):
    import hipddsp
    from ddsp.hubert import n_frames
    for T, want in zip(HC.FRAME_LENGTHS, fix["frames"]):
        got = hipddsp.hubert_frames(T)
        assert got == max(int(want), 0), (T, got, want)
        if want <= 0:
            with pytest.raises(ValueError):
                n_frames(T)
        else:
            assert n_frames(T) == want
    assert hipddsp.hubert_frames(-1) == -1


def test_short_audio_raises_value_error(lib_path):
    from ddsp.hubert import n_frames
    with pytest.raises(ValueError):
        n_frames(100)


def test_cpu_tensor_raises():
    from ddsp.hubert import HubertSoft
    with pytest.raises(RuntimeError):
        HubertSoft().units(torch.zeros(1, 1, 8000))


def test_unsupported_encoders_raise():
    from ddsp.vocoder import Units_Encoder
    for name in ("hubertbase", "hubertbase768", "contentvec", "contentvec768", "xunit", "yunit"):
        with pytest.raises(NotImplementedError, match="hubertsoft"):
            Units_Encoder(name, "unused.pt")
    with pytest.raises(ValueError):
        Units_Encoder("no-such-encoder", "unused.pt")


def test_eager_restatement_matches_the_reference_fp64(fix):
    """The network as this project reads it (hubert_cases.eager_units, fp64 on the CPU) equals the reference's fp64 units."""
    sd = {k: v.double() for k, v in HC.fill(_mirror_shapes()).items()}
    got = HC.eager_units(sd, HC.audio("short").double())
    want = torch.from_numpy(fix["units64_short"]).double()
    err = float(((got - want) ** 2).mean().sqrt() / (want ** 2).mean().sqrt())
    assert err < 1e-7, f"relative rms {err:.3e}"
