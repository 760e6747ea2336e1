"""The autocorrelation f0 extractor on the host: the name, the geometry out of the library against the restatement of
tests/f0_ac_cases.py, the padding arithmetic, the refusals before any launch, and the restatement itself (it finds a tone; its
fp32 form stays within the cap that the GPU test's tolerance is derived from)."""
import numpy as np
import pytest

import f0_ac_cases as AC

# 4 x the largest relative f0 difference between the fp32 and the fp64 restatement over the signals of AC.signals at the three
# geometries (measured: 2.1e-7 at 16 kHz, 5.3e-7 at 44.1 kHz, 6.2e-7 at 48 kHz); the GPU test's tolerance on agreeing frames
F0_RTOL = 2.5e-6
DUR = 0.5


def test_ac_is_accepted_and_cpu_names_still_raise(monkeypatch):
    import torch
    from ddsp.vocoder import F0_Extractor
    for name in ("parselmouth", "dio", "harvest"):
        with pytest.raises(NotImplementedError, match="crepe"):
            F0_Extractor(name, 44100, 512, 65, 800)
    with pytest.raises(ValueError, match="Unknown f0 extractor"):
        F0_Extractor("autocorrelation", 44100, 512, 65, 800)
    # 'ac' passes the name check: without a HIP device the next refusal is the missing device, with one it constructs
    if torch.cuda.is_available():
        assert F0_Extractor("ac", 44100, 512, 65, 800).f0_extractor == "ac"
    else:
        with pytest.raises(RuntimeError, match="HIP device"):
            F0_Extractor("ac", 44100, 512, 65, 800)
    with pytest.raises(RuntimeError, match="HIP device"):
        F0_Extractor("ac", 44100, 512, 65, 800, device="cpu")


@pytest.mark.parametrize("sr,f0_min,f0_max,W,nfft,C", [(44100, 65, 800, 2032, 4096, 15), (48000, 50, 1100, 2878, 8192, 22),
                                                     (16000, 65, 800, 736, 2048, 15)])
def test_sizes_of_the_worked_examples(sr, f0_min, f0_max, W, nfft, C):
    g = AC.geometry(sr, f0_min, f0_max)
    assert (g["W"], g["nfft"], g["C"]) == (W, nfft, C)


@pytest.mark.parametrize("geo", list(AC.GEOMETRIES))
def test_frame_counts_out_of_the_library(lib_path, geo):
    import hipddsp
    sr, hop, f0_min, _ = AC.GEOMETRIES[geo]
    lo = AC.min_samples(sr, hop, f0_min)
    for N in list(range(lo - 3, lo + 3)) + [lo + hop - 1, lo + hop, 5 * hop, 10 * hop + 1, int(1.54 * sr), 30 * sr]:
        want = max(0, AC.ac_frames(N, sr, hop, f0_min))
        assert hipddsp.f0_ac_frames(N, sr, hop, f0_min) == want, N
    assert hipddsp.f0_ac_frames(lo - 1, sr, hop, f0_min) == 0 and hipddsp.f0_ac_frames(lo, sr, hop, f0_min) == 1
    # the window of the worked examples: the shortest row is the first with 3 / f0_min seconds
    assert lo == int(np.ceil(3.0 / f0_min * sr - 1e-9))


@pytest.mark.parametrize("geo", list(AC.GEOMETRIES))
def test_padding_fills_n_frames_exactly(geo):
    sr, hop, f0_min, _ = AC.GEOMETRIES[geo]
    lo = AC.min_samples(sr, hop, f0_min)
    for m in range(lo // hop + 1, lo // hop + 40):
        for N in (m * hop - 1, m * hop, m * hop + 1, m * hop + hop // 2):
            nF = AC.ac_frames(N, sr, hop, f0_min)
            n_frames = N // hop + 1
            pad = AC.pad_frames(N, nF, hop)
            assert nF >= 1 and pad >= 0 and n_frames - nF - pad >= 0, (N, nF, pad)
            # every window lies inside the row
            g = AC.geometry(sr, f0_min, 800)
            first, last = AC.frame_left(N, nF, 0, sr, hop), AC.frame_left(N, nF, nF - 1, sr, hop)
            assert first + 1 - g["half"] >= 0 and last + 1 - g["half"] + g["W"] <= N, (N, first, last)


def test_short_rows_raise_before_any_launch(lib_path):
    import hipddsp
    sr, hop, f0_min, _ = AC.GEOMETRIES["44k"]
    lo = AC.min_samples(sr, hop, f0_min)
    assert hipddsp.check_f0_ac_n_samples([lo, 4000], 2, 4000, sr, hop, f0_min) == [lo, 4000]
    with pytest.raises(ValueError, match=r"n_samples\[1\] = %d .* analysis window" % (lo - 1)):
        hipddsp.check_f0_ac_n_samples([4000, lo - 1], 2, 4000, sr, hop, f0_min)
    with pytest.raises(ValueError):
        AC.analyse(np.zeros(lo - 1), sr, hop, f0_min, 800)
    import preprocess

    class Ext:
        f0_extractor = "ac"

        def min_samples(self):
            return lo
    Ext.sample_rate, Ext.hop_size, Ext.f0_min = sr, hop, f0_min
    preprocess._check_lengths([lo, 3 * lo], sr, hop, None, Ext())
    with pytest.raises(ValueError, match=r"waves\[1\].*'ac'"):
        preprocess._check_lengths([3 * lo, lo - 1], sr, hop, None, Ext())
    with pytest.raises(ValueError, match=r"fewer than 3 CREPE frames"):
        preprocess._check_lengths([300], sr, hop, None)


@pytest.fixture(scope="module")
def both():
    """{(geometry, signal): (fp64 analysis, fp32 analysis, truth per sample or None, frame centres)} - computed once."""
    out = {}
    for geo, (sr, hop, f0_min, f0_max) in AC.GEOMETRIES.items():
        for name, (x, truth) in AC.signals(sr, DUR).items():
            r64 = AC.analyse(x, sr, hop, f0_min, f0_max, np.float64)
            r32 = AC.analyse(x, sr, hop, f0_min, f0_max, np.float32)
            nF = len(r64["f0"])
            cen = np.array([AC.frame_left(len(x), nF, i, sr, hop) for i in range(nF)])
            out[geo, name] = (r64, r32, truth, cen)
    return out


def test_restatement_finds_the_tones(both):
    for (geo, name), (r64, _, truth, cen) in both.items():
        v = r64["f0"] > 0
        if truth is None:       # tone | silence | noise | tone: the silent and the noisy quarters are unvoiced
            q = len(v) // 4
            assert v[:q - 2].all() and v[-q + 2:].all() and not v[q + 3:3 * q - 3].any(), (geo, v)
            assert np.max(np.abs(r64["f0"][v] / 220.0 - 1)) < 5e-3      # (frames at a segment edge see half a tone)
            continue
        assert v.all(), (geo, name)
        err = float(np.max(np.abs(r64["f0"] / truth[cen] - 1)))
        print(f"{geo} {name}: fp64 restatement against the truth, max relative error {err:.2e}")
        # a stationary tone to 1e-4 (the octave trap at its fundamental, not the stronger second harmonic); the glide to the
        # change of its frequency over one window
        assert err < (3e-3 if name == "glide" else 1e-4), (geo, name, err)


def test_fp32_restatement_within_the_cap(both):
    worst = 0.0
    for (geo, name), (r64, r32, _, _) in both.items():
        dis = (r64["choice"] != r32["choice"]) | ((r64["f0"] > 0) != (r32["f0"] > 0))
        assert dis.mean() <= 0.01, (geo, name, int(dis.sum()))
        ok = ~dis & (r64["f0"] > 0)
        rel = float(np.max(np.abs(r32["f0"][ok] / r64["f0"][ok] - 1))) if ok.any() else 0.0
        print(f"{geo} {name}: fp32 against fp64 restatement, {int(dis.sum())} of {len(dis)} frames differ, f0 rel {rel:.2e}")
        worst = max(worst, rel)
    assert worst <= F0_RTOL / 4 * 1.01 and worst >= F0_RTOL / 8, worst     # the constant is 4 x this measurement
