"""`preprocess.analyse_batch` / `preprocess.preprocess` on the host with stand-in analysers (plain objects with the three
`extract` / `encode` signatures that compute on the CPU): grouping, input order, per-file trimming, the host tail of the
reference's preprocess.py:80-91 against a direct numpy restatement, the use_vuv switch, the file tree and f0_stats.npy."""
import os

import numpy as np
import pytest
import torch

import preprocess as PP

SR, HOP = 44100, 512


class Volume:
    """Block RMS without padding subtleties: frame i = sqrt(mean(x[i*hop:(i+1)*hop]^2)) over the row's own samples."""
    hop_size = HOP

    def __init__(self):
        self.calls = []

    def extract(self, audio, n_samples=None):
        self.calls.append((tuple(audio.shape), None if n_samples is None else list(n_samples)))
        counts = [audio.shape[1]] * audio.shape[0] if n_samples is None else n_samples
        out = torch.zeros(audio.shape[0], max(counts) // HOP + 1)
        for b, n in enumerate(counts):
            for i in range(n // HOP + 1):
                blk = audio[b, i * HOP:min((i + 1) * HOP, n)]
                out[b, i] = float(np.sqrt(np.mean(blk.numpy() ** 2))) if len(blk) else 0.0
        return out


class F0:
    """Voiced where the block's mean is above 0.25: f0 = 100 + 400 * mean, else 0."""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def extract(self, audio, uv_interp=False, n_samples=None):
        assert uv_interp is False
        self.calls.append((tuple(audio.shape), None if n_samples is None else list(n_samples)))
        counts = [audio.shape[1]] * audio.shape[0] if n_samples is None else n_samples
        out = torch.zeros(audio.shape[0], max(counts) // HOP + 1)
        for b, n in enumerate(counts):
            for i in range(n // HOP + 1):
                blk = audio[b, i * HOP:min((i + 1) * HOP, n)]
                m = float(blk.mean()) if len(blk) else 0.0
                out[b, i] = 100.0 + 400.0 * m if m > 0.25 else 0.0
        return out


class Units:
    encoder_sample_rate = 16000

    def encode(self, audio, sample_rate, hop_size, n_samples=None):
        assert (sample_rate, hop_size) == (SR, HOP)
        counts = [audio.shape[1]] * audio.shape[0] if n_samples is None else n_samples
        out = torch.zeros(audio.shape[0], max(counts) // HOP + 1, 4)
        for b, n in enumerate(counts):
            k = n // HOP + 1
            out[b, :k] = torch.arange(k)[:, None] + torch.tensor([0.0, 0.25, 0.5, float(n)])
        return out


def _level_wave(levels, extra=0):
    """A wave whose block i has the constant value levels[i]; len = (len(levels) - 1) * HOP + extra (the last block is short)."""
    x = np.concatenate([np.full(HOP, v, dtype=np.float32) for v in levels[:-1]] + [np.full(extra, levels[-1], dtype=np.float32)])
    return x


def _tail(f0, use_vuv):
    """The reference's tail, restated directly."""
    f0 = f0.copy()
    uv = f0 == 0
    if (~uv).any():
        mean = np.mean(np.log(f0[~uv]))
        if not use_vuv:
            f0[uv] = np.interp(np.where(uv)[0], np.where(~uv)[0], f0[~uv])
        return f0, mean, True
    return f0, np.nan, False


VOICED = [0.5, 0.6, 0.7, 0.5, 0.9, 0.4]
GAPS = [0.0, 0.1, 0.5, 0.0, 0.0, 0.8, 0.6, 0.0, 0.1]
UNVOICED = [0.0, 0.1, 0.2, 0.0]


def _waves():
    return [_level_wave(VOICED, 300), _level_wave(GAPS, 400), _level_wave(UNVOICED, 500), _level_wave(VOICED[::-1], 301)]


def test_f0_tail_on_hand_made_contours():
    for c in ([220.0, 230, 240, 250], [0, 0, 200, 0, 0, 260, 250, 0, 0], [0.0, 0, 0]):
        c = np.array(c, dtype=np.float32)
        for use_vuv in (False, True):
            got, mean, voiced = PP.f0_tail(c, use_vuv)
            want, wmean, wvoiced = _tail(c, use_vuv)
            np.testing.assert_array_equal(got, want)
            assert voiced is wvoiced and (np.isnan(mean) if not wvoiced else mean == wmean)
            assert got.dtype == c.dtype and got is not c
    filled = PP.f0_tail(np.array([0, 0, 200, 0, 0, 260, 250, 0, 0], dtype=np.float32))[0]
    np.testing.assert_allclose(filled, [200, 200, 200, 220, 240, 260, 250, 250, 250])      # ends held, no clamp
    assert np.array_equal(PP.f0_tail(np.array([0, 0, 200.0, 0]), use_vuv=True)[0], [0, 0, 200.0, 0])


@pytest.mark.parametrize("use_vuv", [False, True])
def test_records_order_trimming_and_both_paths(use_vuv):
    waves = _waves()
    f0x, vol = F0(), Volume()
    solo = PP.analyse_batch(waves, f0x, vol, Units(), SR, HOP, use_vuv=use_vuv)
    assert [c[1] for c in f0x.calls] == [None] * 4 and [c[0][0] for c in vol.calls] == [1] * 4
    f0r, volr = F0(), Volume()
    lengths = [len(w) for w in waves]
    budget = 2 * max(lengths)
    ragged = PP.analyse_batch([torch.from_numpy(w) for w in waves], f0r, volr, Units(), SR, HOP, batch_samples=budget,
                              use_vuv=use_vuv)
    # grouping: sorted by length, two rows of the longest fit the budget
    from infer_offline import group_segments
    groups = group_segments(lengths, budget)
    assert sorted(i for g in groups for i in g) == [0, 1, 2, 3] and len(groups) == 2 and groups[0][0] == 1
    assert [c[1] for c in f0r.calls] == [[lengths[i] for i in g] for g in groups]
    assert [c[0] for c in volr.calls] == [(len(g), lengths[g[0]]) for g in groups]
    for i, (w, a, b) in enumerate(zip(waves, solo, ragged)):
        n = len(w) // HOP + 1
        raw = F0().extract(torch.from_numpy(w)[None])[0].numpy()
        want, mean, voiced = _tail(raw, use_vuv)
        for r in (a, b):
            assert r["f0"].shape == (n,) and r["volume"].shape == (n,) and r["units"].shape == (n, 4)
            np.testing.assert_array_equal(r["f0"], want)
            assert r["voiced"] is voiced and (np.isnan(r["lf0_mean"]) if not voiced else r["lf0_mean"] == mean)
            assert r["units"][0, 3] == len(w) and r["units"][-1, 0] == n - 1          # this file's own row, in input order
        for k in ("f0", "volume", "units"):
            np.testing.assert_array_equal(a[k], b[k])
    assert [r["voiced"] for r in solo] == [True, True, False, True]
    assert (solo[1]["f0"] == 0).any() == use_vuv and not solo[2]["f0"].any()


def test_a_short_file_is_named():
    waves = _waves() + [np.zeros(200, dtype=np.float32)]
    for kw in ({}, {"batch_samples": 100000}):
        with pytest.raises(ValueError, match=r"waves\[4\]"):
            PP.analyse_batch(waves, F0(), Volume(), Units(), SR, HOP, **kw)


@pytest.mark.parametrize("batch_samples", [None, 12000])
def test_preprocess_writes_the_reference_tree(tmp_path, batch_samples):
    from scipy.io import wavfile
    root = str(tmp_path)
    files = {"1/a.wav": _level_wave(VOICED, 300), "1/b.wav": _level_wave(GAPS, 400), "2/c.wav": _level_wave(VOICED[::-1], 301),
             "2/sub/d.wav": _level_wave(UNVOICED, 500)}
    for rel, w in files.items():
        os.makedirs(os.path.dirname(os.path.join(root, "audio", rel)), exist_ok=True)
        wavfile.write(os.path.join(root, "audio", rel), SR, w)
    skipped = PP.preprocess(root, F0(), Volume(), Units(), SR, HOP, device="cpu", gen_stats=True, batch_samples=batch_samples)
    assert skipped == ["2/sub/d.wav"]
    assert os.path.isfile(os.path.join(root, "skip", "2", "sub", "d.wav")) and not os.path.exists(os.path.join(root, "audio", "2", "sub", "d.wav"))
    means = {}
    for rel, w in files.items():
        stem = rel[:-4]
        n = len(w) // HOP + 1
        units = np.load(os.path.join(root, "units", stem + ".0.npy"))
        assert units.shape == (n, 4) and units[0, 3] == len(w)
        if rel == "2/sub/d.wav":
            assert not any(os.path.exists(os.path.join(root, k, stem + ".npy")) for k in ("f0", "f0_stat", "volume"))
            continue
        want, mean, _ = _tail(F0().extract(torch.from_numpy(w)[None])[0].numpy(), False)
        np.testing.assert_array_equal(np.load(os.path.join(root, "f0", stem + ".npy")), want)
        assert np.load(os.path.join(root, "f0_stat", stem + ".npy")) == mean
        assert np.load(os.path.join(root, "volume", stem + ".npy")).shape == (n,)
        means.setdefault(rel.split("/")[0], []).append(mean)
    stats = np.load(os.path.join(root, "f0_stats.npy"), allow_pickle=True).item()
    assert set(stats) == {"1", "2"}
    for spk, m in means.items():
        assert stats[spk] == sum(m) / len(m)


def test_load_wav_scales_pcm_and_mixes_channels(tmp_path):
    from scipy.io import wavfile
    p = str(tmp_path / "x.wav")
    wavfile.write(p, 22050, np.array([[16384, -16384], [32767, 32767], [-32768, 0]], dtype=np.int16))
    x, rate = PP.load_wav(p)
    assert rate == 22050 and x.dtype == np.float32
    np.testing.assert_allclose(x, [0.0, 32767 / 32768, -0.5])
