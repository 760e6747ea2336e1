"""Ragged CREPE (`Crepe.activations(n_samples=)`, `ctx.crepe_decode(n_frames=)`, `ctx.f0_postfilter(n_crepe=, n_out=)`,
`F0_Extractor.extract(n_samples=)`): every row of a padded batch against the CPU restatement of tests/crepe_cases.py run on
THAT ROW ALONE at its own length - never against a call of the library, except where bit equality with the solo call is the
claim (the dither) or the plumbing is pinned (extract).  Every ragged call runs twice, once with NaN past each row's samples
or frames and once with a plausible decoy there; the two results must be identical.

Gates: those of tests/test_gpu_crepe.py - the per-frame arithmetic is the rectangular call's."""
import numpy as np
import pytest
import torch

import crepe_cases as CC
from test_gpu_crepe import GATE, _model, _with_math

pytestmark = pytest.mark.gpu

T16 = 40000
N16 = [160, 1023, 1024, 4000, 6397, 40000]
FRAMES = [3, 13, 13, 51, 80, 501]


@pytest.fixture(scope="module")
def tiny(dev):
    return _model(dev)


@pytest.fixture(scope="module")
def audio():
    rng = np.random.default_rng(77)
    t = np.arange(T16) / 16000.0
    rows = []
    for b in range(len(N16)):
        f = 90.0 * (1 + 0.4 * b) * np.exp(np.log(3.0) * t / t[-1])
        ph = 2 * np.pi * np.cumsum(f) / 16000.0
        rows.append(0.3 * np.sin(ph) + 0.1 * np.sin(2 * ph + 0.3) + 0.02 * rng.standard_normal(T16))
    return torch.from_numpy(np.stack(rows).astype(np.float32))


@pytest.fixture(scope="module")
def oracle(audio):
    """fp64 activations of every row alone at its own length (computed once, never written to)."""
    sd = CC.fill("tiny")
    return [CC.activations64(sd, audio[b:b + 1, :n])[0] for b, n in enumerate(N16)]


def _padded(x, counts, kind, seed=5):
    """x (B, T, ...) with everything past a row's count replaced by NaN or by a decoy (noise of the signal's size)."""
    y = x.clone()
    rng = np.random.default_rng(seed)
    for b, n in enumerate(counts):
        if kind == "nan":
            y[b, n:] = float("nan")
        else:
            y[b, n:] = torch.from_numpy(0.3 * rng.standard_normal(tuple(y[b, n:].shape))).to(y.dtype)
    return y


def test_frame_counts_of_the_batch():
    import hipddsp
    assert [hipddsp.crepe_frames(n) for n in N16] == FRAMES and hipddsp.crepe_frames(T16) == 501
    assert sum(FRAMES) == 661 and sum(FRAMES[:-1]) < 512 < sum(FRAMES)     # the last row straddles the 512-frame pass
    table = hipddsp.crepe_ragged_table(N16)
    assert table[:6] == N16 and table[6:] == [0, 3, 16, 29, 80, 160, 661]


@pytest.mark.parametrize("mode", ["fp32", "split"])
def test_activations_of_every_row_as_if_alone(ctx, dev, tiny, audio, oracle, mode):
    keep = ctx.math
    _with_math(ctx, mode)
    try:
        runs = [tiny.activations(_padded(audio, N16, kind).to(dev), n_samples=N16).cpu() for kind in ("nan", "decoy")]
        full = _model(dev, "full")
        xf = audio[:2, :400]
        got_full = full.activations(_padded(xf, [160, 400], "nan").to(dev), n_samples=[160, 400]).cpu()
    finally:
        ctx.set_math(keep)
    got = runs[0]
    assert tuple(got.shape) == (6, 501, 360)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(runs[0], runs[1]), "the padding's content reached the result"
    errs = {}
    for b, want in enumerate(oracle):
        n = want.shape[0]
        assert n == FRAMES[b]
        errs[b] = float((got[b, :n].double() - want).abs().max())
        assert torch.equal(got[b, n:], torch.zeros_like(got[b, n:])), f"row {b}: the tail is not exactly 0"
    sd_full = CC.fill("full")
    assert tuple(got_full.shape) == (2, 6, 360) and bool(torch.isfinite(got_full).all())
    for b, n in enumerate([160, 400]):
        want = CC.activations64(sd_full, xf[b:b + 1, :n])[0]
        errs[f"full{b}"] = float((got_full[b, :want.shape[0]].double() - want).abs().max())
        assert torch.equal(got_full[b, want.shape[0]:], torch.zeros_like(got_full[b, want.shape[0]:]))
    print(mode, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < GATE[mode], errs


DECODE_N = [1, 2, 3, 316, 511, 512, 513, 832]


@pytest.fixture(scope="module")
def tracks():
    """P (832,), and the two padded (8, 832, 360) batches of bump_track(n, P[:n]): NaN after a row's frames, or a 0.95 bump
    on another bin from the first frame past the row's end on."""
    kp = CC.known_path()
    P = np.concatenate([kp, kp[::-1], kp[:200]])
    assert len(P) == 832
    full = CC.bump_track(len(P), P)
    decoy = CC.bump_track(len(P), (P + 150) % 360)
    nan = np.full((len(DECODE_N), len(P), 360), np.nan, dtype=np.float32)
    dec = np.empty_like(nan)
    for b, n in enumerate(DECODE_N):
        nan[b, :n] = full[:n]
        dec[b, :n] = full[:n]
        dec[b, n:] = decoy[n:]
    return P, full, torch.from_numpy(nan), torch.from_numpy(dec)


def test_decode_returns_the_known_path_of_every_row(ctx, dev, tracks):
    P, full, nan, dec = tracks
    outs = [ctx.crepe_decode(p.to(dev), 50, 1100, segment=512, dither=False, want_bins=True, n_frames=DECODE_N)
            for p in (nan, dec)]
    for a, b in zip(*outs):
        assert torch.equal(a, b), "the padding's content reached the decode"
    f0, pd, bins = (t.cpu().numpy() for t in outs[0])
    assert f0.shape == pd.shape == bins.shape == (8, 832)
    assert np.all(np.isfinite(f0)) and np.all(np.isfinite(pd))
    for b, n in enumerate(DECODE_N):
        np.testing.assert_array_equal(bins[b, :n], P[:n], err_msg=f"row {b} ({n} frames)")
        np.testing.assert_allclose(f0[b, :n], CC.bin_to_hz(P[:n]), rtol=2e-7)
        np.testing.assert_array_equal(pd[b, :n], full[np.arange(n), P[:n]])
        assert not f0[b, n:].any() and not pd[b, n:].any() and not bins[b, n:].any(), f"row {b}: the tail is not 0"


def test_dithered_rows_equal_their_solo_decode(ctx, dev, tracks):
    _, _, nan, dec = tracks
    seed = 0x1234_5678_9ABC
    got = ctx.crepe_decode(nan.to(dev), 50, 1100, segment=512, dither_seed=seed, dither=True, n_frames=DECODE_N)
    again = ctx.crepe_decode(dec.to(dev), 50, 1100, segment=512, dither_seed=seed, dither=True, n_frames=DECODE_N)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
    plain = ctx.crepe_decode(nan.to(dev), 50, 1100, segment=512, dither=False, n_frames=DECODE_N)[0]
    assert not torch.equal(plain, got[0])
    for b, n in enumerate(DECODE_N):
        solo = ctx.crepe_decode(nan[b:b + 1, :n].to(dev), 50, 1100, segment=512, dither_seed=seed, dither=True)
        assert torch.equal(got[0][b, :n], solo[0][0]) and torch.equal(got[1][b, :n], solo[1][0]), f"row {b} ({n} frames)"
        assert not got[0][b, n:].any() and not got[1][b, n:].any()


PF_CREPE = [3, 400, 57, 123, 250, 399]


def _n_out(fr, sr, hop):
    """Output frames as `extract` computes them for the `sr` samples that give (fr - 1) * 80 + 40 samples at 16 kHz."""
    n = int(((fr - 1) * 80 + 40) * sr / 16000)
    return int(n // hop) + 1


@pytest.mark.parametrize("sr,hop", [(44100, 512), (48000, 512 * 48000 / 44100)])
@pytest.mark.parametrize("uv_interp", [False, True])
def test_postfilter_of_every_row_as_if_alone(ctx, dev, sr, hop, uv_interp):
    rng = np.random.default_rng(11)
    f0 = rng.uniform(60, 900, (6, 400)).astype(np.float32)
    pd = rng.uniform(0, 0.3, (6, 400)).astype(np.float32)      # ~1/6 of the frames below the 0.05 threshold
    pd[2] = rng.uniform(0, 0.04, 400)                          # a row with no voiced frame
    pd[3, PF_CREPE[3] - 20:PF_CREPE[3]] = 0.01                 # a row that ends unvoiced
    n_out = [_n_out(fr, sr, hop) for fr in PF_CREPE]
    outs = []
    for kind in ("nan", "decoy"):
        f, p = torch.from_numpy(f0).clone(), torch.from_numpy(pd).clone()
        for b, fr in enumerate(PF_CREPE):
            f[b, fr:] = float("nan") if kind == "nan" else 440.0
            p[b, fr:] = float("nan") if kind == "nan" else 0.9
        outs.append(ctx.f0_postfilter(f.to(dev), p.to(dev), sr, hop, max(n_out), 0, 0.05, uv_interp, 65.0,
                                      n_crepe=PF_CREPE, n_out=n_out).cpu())
    assert torch.equal(outs[0], outs[1]), "the padding's content reached the post-filter"
    got = outs[0].numpy()
    assert got.shape == (6, max(n_out)) and np.all(np.isfinite(got))
    for b, fr in enumerate(PF_CREPE):
        want = CC.postfilter(f0[b, :fr], pd[b, :fr], sr, hop, n_out[b], 0, uv_interp, 65.0)
        row = got[b, :n_out[b]]
        ulp = np.abs(row.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, (b, int(ulp.max()), int((ulp > 0).sum()))
        assert not got[b, n_out[b]:].any(), f"row {b}: the tail is not 0"
    if not uv_interp:
        assert not got[2].any()                                # (the all-unvoiced row stays unvoiced)


def _sweep(sr, n, f=150.0, seed=0):
    t = np.arange(n) / sr
    rng = np.random.default_rng(seed)
    return (0.3 * np.sin(2 * np.pi * f * t * (1 + 0.3 * t)) + 0.01 * rng.standard_normal(n)).astype(np.float32)


def test_extract_is_the_chain_of_the_ragged_calls(ctx, dev, tiny):
    import hipddsp
    from ddsp.vocoder import F0_Extractor
    ex = F0_Extractor("crepe", 44100, 512, 65, 800, crepe_ckpt=tiny, device=dev)
    counts = [30000, 441, 52920]
    T = max(counts)
    x = torch.zeros(3, T)
    for b, n in enumerate(counts):
        x[b, :n] = torch.from_numpy(_sweep(44100, n, 140.0 + 60 * b, b))
    outs = [ex.extract(_padded(x, counts, kind).to(dev), uv_interp=True, dither=False, n_samples=counts) for kind in ("nan", "decoy")]
    assert torch.equal(outs[0], outs[1])
    got = outs[0]
    n_out = [n // 512 + 1 for n in counts]
    assert got.is_cuda and tuple(got.shape) == (3, T // 512 + 1)
    assert bool(torch.isfinite(got).all())
    for b, n in enumerate(n_out):
        assert bool((got[b, :n] >= 65).all()) and not got[b, n:].any()
    # the same launches, composed here
    lib = hipddsp.load_library()
    n16 = [int(lib.ddsp_resample_length(n, 44100, 16000)) for n in counts]
    n_crepe = [hipddsp.crepe_frames(n) for n in n16]
    xd = _padded(x, counts, "nan").to(dev)
    x16 = ctx.resample(xd, 44100, 16000, lowpass_filter_width=128, n_dev=ctx.ragged_counts(counts))
    probs = tiny.activations(x16, n_samples=n16)
    f0, pd = ctx.crepe_decode(probs, 65, 800, segment=512, dither=False, n_frames=n_crepe)
    want = ctx.f0_postfilter(f0, pd, 44100, 512, max(n_out), 0, 0.05, True, 65, n_crepe=n_crepe, n_out=n_out)
    assert torch.equal(got, want)
    # dithered by default, seeded
    a = ex.extract(xd, n_samples=counts, seed=9)
    assert torch.equal(a, ex.extract(xd, n_samples=counts, seed=9)) and not torch.equal(a, ex.extract(xd, n_samples=counts, seed=10))


def test_refusals(ctx, dev, tiny):
    from ddsp.vocoder import F0_Extractor
    ex = F0_Extractor("crepe", 44100, 512, crepe_ckpt=tiny, device=dev)
    x = torch.zeros(2, 44100, device=dev)
    # 438 samples are ceil(438 * 16000 / 44100) = 159 at 16 kHz: 2 CREPE frames; 439 are 160: 3 frames, the shortest accepted
    for bad in ([0, 44100], [44101, 44100], [438, 44100], torch.tensor([44100, 44100], device=dev), [44100],
                [44100.0, 44100]):
        with pytest.raises(ValueError):
            ex.extract(x, n_samples=bad)
    ex.extract(x, n_samples=[439, 44100])
    with pytest.raises(ValueError):
        ex.extract(x, silence_front=0.5, n_samples=[44100, 44100])
    with pytest.raises(ValueError):
        ex.extract(x, seed_dev=torch.zeros(1, dtype=torch.int64, device=dev), n_samples=[44100, 44100])
    x16 = torch.zeros(2, 16000, device=dev)
    for bad in ([0, 16000], [16001, 16000], [159, 16000], torch.tensor([16000, 16000], device=dev)):
        with pytest.raises(ValueError):
            tiny.activations(x16, n_samples=bad)
    probs = torch.zeros(2, 10, 360, device=dev)
    for bad in ([0, 10], [11, 10], torch.tensor([10, 10], device=dev)):
        with pytest.raises(ValueError):
            ctx.crepe_decode(probs, 50, 1100, n_frames=bad)
    with pytest.raises(ValueError):
        ctx.crepe_decode(probs, 50, 1100, n_frames=[10, 10], seed_dev=torch.zeros(1, dtype=torch.int64, device=dev))
    f = torch.zeros(2, 10, device=dev)
    for kw in (dict(n_crepe=[2, 10], n_out=[5, 5]), dict(n_crepe=[10, 11], n_out=[5, 5]), dict(n_crepe=[10, 10], n_out=[0, 5]),
               dict(n_crepe=[10, 10], n_out=[6, 5]), dict(n_crepe=[10, 10]), dict(n_crepe=[10, 10], n_out=[5, 5], start_frame=1)):
        kw = dict(kw)
        start = kw.pop("start_frame", 0)
        with pytest.raises(ValueError):
            ctx.f0_postfilter(f, f, 44100, 512, 5, start, n_crepe=kw.get("n_crepe"), n_out=kw.get("n_out"))
