"""One row-length rule per analyser (ddsp/analysis.py): for the volume, the units encoder and both f0 back ends, `min_samples()`
is accepted and `min_samples() - 1` refused, in the analyser's own words, by the ragged check of the public call and by
`preprocess._check_lengths` alike; and `_check_lengths` takes the rule from the analyser it is given, whatever its name.

No device: the analysers are built around CPU tensors, where a ragged call whose counts pass ends in the 'HIP device only'
RuntimeError and one whose counts do not is refused before that (ValueError)."""
import re

import pytest
import torch


class _Any:
    """An analyser that accepts every file."""
    too_short = "are never too short"

    def min_samples(self, *args):
        return 1


def _f0(name, sr, hop, f0_min):
    from ddsp import analysis as A
    from ddsp.crepe import Crepe
    ext = A.F0_Extractor.__new__(A.F0_Extractor)     # (the constructor wants a HIP device)
    ext.f0_extractor, ext.sample_rate, ext.hop_size, ext.device = name, sr, hop, "cpu"
    ext.back_end = A.F0_Extractor._BACK_ENDS[name](sr, hop, f0_min, 800, Crepe("tiny"), "cpu")
    return ext


def _case(kind, sr, hop):
    """-> (min_samples, ragged(n): the public ragged call on one row of n samples, files(n): _check_lengths on one file,
    the ragged refusal's words, the file refusal's words)."""
    import preprocess
    from ddsp import analysis as A
    if kind == "volume":
        vol = A.Volume_Extractor(hop, device="cpu")
        return (vol.min_samples(), lambda n: vol.extract(torch.zeros(1, n), n_samples=[n]),
                lambda n: preprocess._check_lengths([n], sr, hop, _Any(), _Any()),
                "samples are not longer than the reflect padding 256", "are not longer than the volume's reflect padding 256")
    if kind == "units":
        enc = A.Units_Encoder.__new__(A.Units_Encoder)     # (the constructor wants a checkpoint file)
        enc.encoder_sample_rate, enc.encoder_hop_size = 16000, 320
        return (enc.min_samples(sr), lambda n: enc.encode(torch.zeros(1, n), sr, hop, n_samples=[n]),
                lambda n: preprocess._check_lengths([n], sr, 1, enc, _Any()),
                "samples are too short for the conv stack", "are too short for the units encoder's conv stack")
    ext = _f0(kind, sr, hop, 65)
    words = {"crepe": ("samples at 16 kHz give 2 CREPE frames; the reflect-padded filters need at least 3",
                       "give fewer than 3 CREPE frames"),
             "ac": (f"samples at {sr} Hz are shorter than one analysis window of 3 / f0_min = {3.0 / 65:.4f} s",
                    f"are shorter than one analysis window of the 'ac' f0 extractor ({ext.min_samples()} samples)")}[kind]
    return (ext.min_samples(), lambda n: ext.extract(torch.zeros(1, n), n_samples=[n]),
            lambda n: preprocess._check_lengths([n], sr, 1, _Any(), ext), *words)


# (the shortest rows, worked by hand: 257 > (512 + 1) // 2; 320 samples at 16 kHz give one encoder frame and 880 at 44.1 kHz are
# 320; 160 samples at 16 kHz give 3 CREPE frames and 439 at 44.1 kHz are 160; 3 / 65 s are 2035.4 and 738.5 samples)
CASES = [("volume", 44100, 512, 257), ("units", 16000, 160, 320), ("units", 44100, 512, 880), ("crepe", 44100, 512, 439),
         ("crepe", 16000, 160, 160), ("ac", 44100, 512, 2036), ("ac", 16000, 160, 739)]


@pytest.mark.parametrize("kind,sr,hop,want", CASES)
def test_the_minimum_is_accepted_and_one_less_refused_in_the_analysers_words(lib_path, kind, sr, hop, want):
    lo, ragged, files, row_words, file_words = _case(kind, sr, hop)
    assert lo == want
    with pytest.raises(RuntimeError, match="HIP device"):      # the counts passed: the next refusal is the missing device
        ragged(lo)
    files(lo)
    with pytest.raises(ValueError, match=re.escape(f"n_samples[0] = ") + r"\d+ " + re.escape(row_words)):
        ragged(lo - 1)
    with pytest.raises(ValueError, match=re.escape(f"waves[0]: {lo - 1} samples {file_words}")):
        files(lo - 1)


def test_check_lengths_takes_the_rule_from_the_analyser_it_is_given(lib_path):
    import preprocess

    class Made_Up:
        f0_extractor = "crepe"     # (a name decides nothing)
        too_short = "are fewer than this back end wants"

        def min_samples(self):
            return 12345
    preprocess._check_lengths([12345, 99999], 44100, 512, None, Made_Up())
    with pytest.raises(ValueError, match=r"waves\[1\]: 12344 samples are fewer than this back end wants"):
        preprocess._check_lengths([12345, 12344], 44100, 512, None, Made_Up())
    # the defaults: no units encoder is the HuBERT-Soft rule at its own rate, no f0 extractor the CREPE rule
    preprocess._check_lengths([880], 44100, 512, None, _Any())
    with pytest.raises(ValueError, match="units encoder's conv stack"):
        preprocess._check_lengths([879], 44100, 512, None, _Any())
    preprocess._check_lengths([880], 44100, 512, None)
    with pytest.raises(ValueError, match="fewer than 3 CREPE frames"):
        preprocess._check_lengths([438], 44100, 512, _Any())
