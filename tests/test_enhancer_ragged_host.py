"""Ragged NSF-HiFiGAN enhancer, host side (no GPU): the new entry points are exported, declared and bound; the counts are
checked before any device work; `enhancer_batch_samples` is where the issue puts it; and the host integers behind
`enhance_batch`'s `n_out` are those a solo `enhance` goes through."""
import inspect
import json
import os
import re

import pytest
import torch

import glue_cases as GC
from conftest import ROOT
from oracle import enhancer as OE
from oracle import resample as OR

NEW = ["ddsp_conv1d", "ddsp_conv1d_pair", "ddsp_nsf_source", "ddsp_nsf_noise_conv", "ddsp_nsf_post", "ddsp_stft_frames",
       "ddsp_retime_f0"]


class _OnDevice(torch.Tensor):
    """A tensor that reports `is_cuda` (there is no device on this side of the suite)."""
    is_cuda = property(lambda self: True)


def test_new_symbols_are_exported_declared_and_bound(lib_path):
    import hipddsp
    lib = hipddsp.load_library()
    with open(os.path.join(ROOT, "include", "ddsp_amd.h")) as fh:
        header = fh.read()
    for name in NEW:
        assert name in hipddsp.SIGNATURES, name
        assert getattr(lib, name).argtypes == hipddsp.SIGNATURES[name][1]
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in include/ddsp_amd.h"
        assert len(decl.group(1).split(",")) == len(hipddsp.SIGNATURES[name][1]), name
    # one binding method per operation: the ragged form is an argument of the un-suffixed method
    for m, names in (("nsf_source", ["n_dev"]), ("nsf_post", ["rows"]), ("retime_f0", ["n_src_dev", "n_dst_dev"])):
        for n in names:
            assert inspect.signature(getattr(hipddsp.Context, m)).parameters[n].default is None, (m, n)
    for m in ("nsf_noise_conv", "stft_frames"):
        assert hasattr(hipddsp.Context, m), m
    assert not [a for a in dir(hipddsp.Context) if a.endswith("_ragged")]
    for m in ("conv1d", "conv1d_pair"):
        assert inspect.signature(getattr(hipddsp.Context, m)).parameters["rows"].default is None


def test_abi_versions_agree(lib_path):
    import hipddsp
    with open(os.path.join(ROOT, "ddsp-svc-official_amd", "csrc", "ctx.hip")) as fh:
        src = int(re.search(r"#define DDSP_ABI_VERSION (\d+)", fh.read()).group(1))
    assert hipddsp.ABI_VERSION == src == hipddsp.load_library().ddsp_abi_version()


def test_enhancer_batch_samples_is_a_keyword_of_render_and_convert_batched():
    """Last in `render`; in `convert_batched` it stands before `units_batch_samples`, which an earlier test pins as last."""
    import infer_offline
    params = list(inspect.signature(infer_offline.render).parameters.values())
    assert params[-1].name == "enhancer_batch_samples" and params[-1].default is None
    p = inspect.signature(infer_offline.convert_batched).parameters
    assert p["enhancer_batch_samples"].default is None and list(p).index("enhancer_batch_samples") >= 9     # keyword use only
    assert "enhancer_batch_samples" not in inspect.signature(infer_offline.convert).parameters
    from enhancer import Enhancer
    assert list(inspect.signature(Enhancer.enhance).parameters) == ["self", "audio", "sample_rate", "f0", "hop_size", "adaptive_key",
                                                                    "silence_front", "rand_ini"]
    assert list(inspect.signature(Enhancer.enhance_batch).parameters)[:8] == ["self", "audio", "sample_rate", "f0", "hop_size",
                                                                              "n_samples", "adaptive_key", "rand_ini"]
    assert "silence_front" not in inspect.signature(Enhancer.enhance_batch).parameters


def _enhancer(tmp_path):
    from enhancer import Enhancer
    with open(tmp_path / "config.json", "w") as fh:
        json.dump(dict(GC.NSF_CONFIG), fh)
    torch.save({"generator": GC.nsf_state_dict()}, tmp_path / "model")
    return Enhancer("nsf-hifigan", str(tmp_path / "model"), device="cpu")


def test_bad_counts_raise_before_any_device_work(lib_path, tmp_path):
    """CPU tensors: a valid call ends in the 'HIP device only' RuntimeError; bad counts must be refused first."""
    from enhancer import AttrDict, Generator, STFT
    h = GC.NSF_CONFIG
    gen = Generator(AttrDict(h), GC.nsf_state_dict())
    st = STFT(h["sampling_rate"], h["num_mels"], h["n_fft"], h["win_size"], h["hop_size"], h["fmin"], h["fmax"])
    enh = _enhancer(tmp_path)
    N = 640
    mel, f0 = torch.zeros(3, h["num_mels"], N), torch.zeros(3, N)
    audio, track = torch.zeros(3, N), torch.zeros(3, 20, 1)
    bad = [[N, N], [N] * 4, [0, N, N], [N, N + 1, N], [N, -5, N], torch.tensor([N, N, N]).as_subclass(_OnDevice), [float(N), N, N],
           [True, N, N], N, torch.tensor([[N, N, N]])]
    for n in bad:
        for call in (lambda: gen(mel, f0, n_frames=n), lambda: st.get_mel(audio, n_samples=n),
                     lambda: enh.enhancer(audio, f0, n_samples=n), lambda: enh.enhance_batch(audio, 44100, track, 32, n)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        enh.enhance_batch(audio, 44100, track, 32, [N, N, N], n_f0=[20, 21, 20])
    for call in (lambda: gen(mel, f0, n_frames=[N, 7, 1]), lambda: gen(mel, f0), lambda: st.get_mel(audio, n_samples=[N, 70, 1]),
                 lambda: st.get_mel(audio), lambda: enh.enhance_batch(audio, 44100, track, 32, [N, 70, 1])):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()


def test_host_lengths_are_the_solo_lengths(lib_path, tmp_path):
    """`STFT.frame_count` against the frames `OE.log_mel` returns for every length from 1 to 3 * n_fft, and
    `Enhancer.batch_lengths` against the lengths of `oracle.resample` in and out for keys 0, 4 and 7."""
    from enhancer import mel_filterbank
    h = GC.NSF_CONFIG
    enh = _enhancer(tmp_path)
    st = enh.enhancer.stft()
    basis = torch.from_numpy(mel_filterbank(h["sampling_rate"], h["n_fft"], h["num_mels"], h["fmin"], h["fmax"]))
    hop = h["hop_size"]
    for T in range(1, 3 * h["n_fft"] + 1):
        frames = OE.log_mel(torch.zeros(1, T), h, basis).shape[-1]
        assert st.frame_count(T) == frames, T
        assert enh.batch_lengths(T, 44100, 44100) == (T, T // hop + 1, frames, frames * hop, frames * hop), T
    for key in (0, 4, 7):
        rate, _, _ = enh._working_rate(key, None)
        for T in (1, 33, 1000, 4096):
            a = torch.zeros(1, T) if rate == 44100 else OR.resample(torch.zeros(1, T), 44100, rate, 128)
            frames = OE.log_mel(a, h, basis).shape[-1]
            back = frames * hop if rate == 44100 else OR.resample(torch.zeros(1, frames * hop), rate, 44100, 128).shape[-1]
            assert enh.batch_lengths(T, 44100, rate) == (a.shape[-1], a.shape[-1] // hop + 1, frames, frames * hop, back), (key, T)
