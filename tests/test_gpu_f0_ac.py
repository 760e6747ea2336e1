"""`F0_Extractor('ac')` / `ctx.f0_ac` on the device against the fp64 restatement of tests/f0_ac_cases.py (never against a call of
the library, except where bit equality with another call is the claim: ragged rows, graph replay, the real-time chain).

Gates.  On frames where the device and the fp64 restatement agree on the voicing and on the chosen candidate, f0 agrees to
F0_RTOL = 2.5e-6: 4 x the largest relative difference between the fp32 and the fp64 restatement on these signals (6.2e-7,
tests/test_f0_ac_host.py measures it on the CPU); the margin covers the kernel's FFT summation order.  At most 2 % of a signal's
frames may disagree (near-ties in the path or at a threshold; the fp32 restatement itself disagrees on none of them).  Against the
ground truth of the stationary tones and the glide the device gets twice the fp64 restatement's own error."""
import numpy as np
import pytest
import torch

import f0_ac_cases as AC
from test_f0_ac_host import DUR, F0_RTOL

pytestmark = pytest.mark.gpu
GEOS = list(AC.GEOMETRIES)


@pytest.fixture(scope="module")
def cases():
    """{geometry: {signal: (x, truth, fp64 analysis)}} - computed once, never written to."""
    out = {}
    for geo, (sr, hop, f0_min, f0_max) in AC.GEOMETRIES.items():
        out[geo] = {name: (x, truth, AC.analyse(x, sr, hop, f0_min, f0_max)) for name, (x, truth) in AC.signals(sr, DUR).items()}
    return out


def _extractor(geo, dev):
    from ddsp.vocoder import F0_Extractor
    sr, hop, f0_min, f0_max = AC.GEOMETRIES[geo]
    return F0_Extractor("ac", sr, hop, f0_min, f0_max, device=dev)


def _compare(tag, f0, choice, ref):
    nF = len(ref["f0"])
    f0, choice = f0[:nF].astype(np.float64), choice[:nF]
    dis = (choice != ref["choice"]) | ((f0 > 0) != (ref["f0"] > 0))
    ok = ~dis & (ref["f0"] > 0)
    rel = float(np.max(np.abs(f0[ok] / ref["f0"][ok] - 1))) if ok.any() else 0.0
    print(f"{tag}: {int(dis.sum())} of {nF} frames differ, {int(ok.sum())} voiced agree, f0 rel {rel:.2e} (gate {F0_RTOL:.1e})")
    assert dis.mean() <= 0.02, (tag, np.where(dis)[0])
    assert rel <= F0_RTOL, (tag, rel)
    return rel


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("geo", GEOS)
def test_against_the_fp64_restatement(ctx, dev, cases, geo, B):
    """The analysis frames (candidate choice, voicing, f0) and the padded track of `extract`."""
    sr, hop, f0_min, f0_max = AC.GEOMETRIES[geo]
    names = ["octave"] if B == 1 else ["tone", "glide", "segments"]
    x = torch.from_numpy(np.stack([cases[geo][n][0] for n in names])).to(dev)
    N = x.shape[1]
    n_frames = N // hop + 1
    raw, choice = ctx.f0_ac(x, sr, hop, f0_min, f0_max, n_frames, want_choice=True)
    ext = _extractor(geo, dev)
    track = ext.extract(x)
    track_i = ext.extract(x, uv_interp=True)
    torch.cuda.synchronize()
    assert torch.equal(raw, track) and track.shape == (B, n_frames)
    for b, n in enumerate(names):
        ref = cases[geo][n][2]
        nF = len(ref["f0"])
        pad = AC.pad_frames(N, nF, hop)
        row = track[b].cpu().numpy()
        assert (row[:pad] == 0).all() and (row[pad + nF:] == 0).all()
        _compare(f"{geo} B={B} {n}", row[pad:pad + nF], choice[b].cpu().numpy(), ref)
        # uv_interp: the reference's interpolation and clamp of the device's own track, to fp32 rounding
        want = AC.uv_interp_clamp(row, f0_min)
        np.testing.assert_allclose(track_i[b].cpu().numpy(), want, rtol=3e-7, atol=0)
    one = ext.extract(x[0])
    assert one.shape == (n_frames,) and torch.equal(one, track[0])
    as_np = ext.extract(cases[geo][names[0]][0])
    assert isinstance(as_np, np.ndarray) and as_np.dtype == np.float32 and np.array_equal(as_np, track[0].cpu().numpy())


@pytest.mark.parametrize("geo", GEOS)
def test_accuracy_against_the_truth(ctx, dev, cases, geo):
    """Stationary tones and the glide: the device's error against the signal's own frequency at the frame centre is within
    twice the fp64 restatement's."""
    sr, hop, f0_min, f0_max = AC.GEOMETRIES[geo]
    for name in ("tone", "octave", "glide"):
        x, truth, ref = cases[geo][name]
        N, nF = len(x), len(ref["f0"])
        cen = np.array([AC.frame_left(N, nF, i, sr, hop) for i in range(nF)])
        got = ctx.f0_ac(torch.from_numpy(x)[None].to(dev), sr, hop, f0_min, f0_max, N // hop + 1)[0].cpu().numpy().astype(np.float64)
        pad = AC.pad_frames(N, nF, hop)
        got = got[pad:pad + nF]
        assert (got > 0).all() and (ref["f0"] > 0).all()
        e_ref = float(np.max(np.abs(ref["f0"] / truth[cen] - 1)))
        e_dev = float(np.max(np.abs(got / truth[cen] - 1)))
        print(f"{geo} {name}: error against the truth, fp64 restatement {e_ref:.2e}, device {e_dev:.2e}")
        assert e_dev <= 2 * e_ref, (geo, name, e_dev, e_ref)


@pytest.mark.parametrize("geo", GEOS)
def test_zeros(dev, geo):
    sr, hop, f0_min, _ = AC.GEOMETRIES[geo]
    ext = _extractor(geo, dev)
    x = torch.from_numpy(AC.zeros(sr, DUR)).to(dev)
    f0, f0_i = ext.extract(x), ext.extract(x, uv_interp=True)
    assert f0.shape == (len(x) // hop + 1,) and (f0 == 0).all() and (f0_i == float(f0_min)).all()


@pytest.mark.parametrize("geo", GEOS)
def test_silence_front(dev, cases, geo):
    """The crop and the padding of the reference: start_frame = int(silence_front * sr / hop) frames of zeros, then the cropped
    audio's own track - the same frames as the crop analysed alone, bit for bit, and the restatement's to the gate."""
    sr, hop, f0_min, f0_max = AC.GEOMETRIES[geo]
    ext = _extractor(geo, dev)
    x = cases[geo]["glide"][0]
    sf = 0.13
    start_frame = int(sf * sr / hop)
    crop = int(np.round(start_frame * hop / sr * sr))
    got = ext.extract(torch.from_numpy(x).to(dev), silence_front=sf)
    alone = ext.extract(torch.from_numpy(x[crop:].copy()).to(dev))
    n_frames = len(x) // hop + 1
    assert got.shape == (n_frames,) and start_frame >= 3
    nF = AC.ac_frames(len(x) - crop, sr, hop, f0_min)
    pad0 = AC.pad_frames(len(x) - crop, nF, hop)
    pad = pad0 + start_frame
    assert (got[:pad] == 0).all() and (got[pad + nF:] == 0).all()
    assert torch.equal(got[pad:pad + nF], alone[pad0:pad0 + nF])
    want = AC.extract(x, sr, hop, f0_min, f0_max, silence_front=sf)
    v = want > 0
    assert np.array_equal(v, got.cpu().numpy() > 0)
    assert np.max(np.abs(got.cpu().numpy()[v] / want[v] - 1)) <= F0_RTOL
    got_i = ext.extract(torch.from_numpy(x).to(dev), uv_interp=True, silence_front=sf).cpu().numpy()
    np.testing.assert_allclose(got_i, AC.uv_interp_clamp(got.cpu().numpy(), f0_min), rtol=3e-7, atol=0)


@pytest.mark.parametrize("uv_interp", [False, True])
@pytest.mark.parametrize("geo", GEOS)
def test_ragged_rows_equal_the_rows_alone(dev, cases, geo, uv_interp):
    """Counts (full, ~60 %, one window + 1 sample): every row equals its solo call bit for bit, is exactly 0 after its own
    frames, and what follows a row's samples (a decoy or NaN) does not matter."""
    sr, hop, f0_min, _ = AC.GEOMETRIES[geo]
    ext = _extractor(geo, dev)
    x = np.stack([cases[geo][n][0] for n in ("glide", "segments", "tone")])
    T = x.shape[1]
    counts = [T, int(0.6 * T) + 1, AC.min_samples(sr, hop, f0_min) + 1]
    outs = []
    for kind in ("decoy", "nan"):
        y = x.copy()
        for b, n in enumerate(counts):
            y[b, n:] = np.nan if kind == "nan" else 0.25
        outs.append(ext.extract(torch.from_numpy(y).to(dev), uv_interp=uv_interp, n_samples=counts))
    assert torch.equal(outs[0], outs[1]) and outs[0].shape == (3, T // hop + 1)
    for b, n in enumerate(counts):
        alone = ext.extract(torch.from_numpy(x[b, :n].copy()).to(dev), uv_interp=uv_interp)
        assert alone.shape == (n // hop + 1,)
        assert torch.equal(outs[0][b, :n // hop + 1], alone), (b, n)
        assert (outs[0][b, n // hop + 1:] == 0).all(), (b, n)
    if not uv_interp:
        assert (outs[0][0] > 0).sum() > 10 and (outs[0][2] > 0).sum() >= 1
    with pytest.raises(ValueError, match="analysis window"):
        ext.extract(torch.from_numpy(x).to(dev), n_samples=[T, T, counts[2] - 2])
    with pytest.raises(ValueError, match="analysis window"):
        ext.extract(torch.from_numpy(x[0, :counts[2] - 2].copy()).to(dev))
    with pytest.raises(ValueError, match="silence_front"):
        ext.extract(torch.from_numpy(x).to(dev), n_samples=counts, silence_front=0.1)


def test_graph_replay_equals_eager(dev, cases):
    sr, hop, f0_min, _ = AC.GEOMETRIES["48k"]
    ext = _extractor("48k", dev)
    xs = [torch.from_numpy(np.stack([cases["48k"][n][0] for n in names])).to(dev)
          for names in (("glide", "segments"), ("tone", "octave"))]
    eager = [ext.extract(x, uv_interp=True, silence_front=0.05, seed_dev=None, dither=True) for x in xs]
    static = xs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ext.extract(static, uv_interp=True, silence_front=0.05)      # (tables and scratch exist before the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ext.extract(static, uv_interp=True, silence_front=0.05)
    for x, want in zip(xs[::-1], eager[::-1]):
        static.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


def test_stream_renderer_block_equals_the_eager_chain(dev, lib_path, tmp_path):
    """`StreamRenderer(..., f0_extractor="ac")`: `push_audio` (one graph replay) against the same chain run eagerly from
    `F0_Extractor('ac').extract` and `push_block(block, units=, f0=)` on an analysis-free renderer, bit for bit."""
    import hubert_cases as HC
    import realtime
    import synthetic
    from ddsp.hubert import HubertSoft
    from ddsp.vocoder import Units_Encoder
    from test_gpu_stream_chain import TIMING
    path = str(tmp_path / "hubert-soft.pt")
    torch.save(HC.fill({k: tuple(v.shape) for k, v in HubertSoft().state_dict().items()}), path)
    encoder = Units_Encoder("hubertsoft", path, device=dev)
    sr, pitch = 44100, 2.0
    block_time, xfade_time, buffer_num = TIMING["config5"]
    model, _ = synthetic.build_model("CombSub", seed=43)
    model = model.to(dev)
    common = dict(buffer_num=buffer_num, threshold_db=-45.0, spk_id=2, use_graph=True, pitch_adjust=pitch)
    r = realtime.StreamRenderer(model, sr, block_time, xfade_time, dev, units_encoder=encoder, f0_extractor="ac", f0_min=65,
                                f0_max=800, **common)
    plain = realtime.StreamRenderer(model, sr, block_time, xfade_time, dev, **common)
    assert r.f0_extractor.f0_extractor == "ac" and (r.f0_extractor.f0_min, r.f0_extractor.f0_max) == (65.0, 800.0)
    assert r.f0_extractor.sample_rate == sr and r.f0_extractor.hop_size == r.hop_size
    window = torch.zeros(r.n_in, device=dev)
    rng = np.random.Generator(np.random.PCG64(91))
    voiced = 0
    for k in range(3):
        t = (np.arange(r.block) + k * r.block) / sr
        blk = torch.from_numpy((0.2 * np.sin(2 * np.pi * 147.0 * t) + 0.01 * rng.standard_normal(r.block)).astype(np.float32)).to(dev)
        noise = synthetic.make_inputs(6000 + k, 1, r.frames)["noise"].to(dev)
        window = torch.cat([window[r.block:], blk])
        f0 = r.f0_extractor.extract(window, uv_interp=True, silence_front=r.silence_front)[None, :, None]
        units = encoder.encode(window[None], sr, r.hop_size)
        em = r.push_audio(blk, noise=noise)
        torch.cuda.synchronize()
        assert torch.equal(r.last_f0, f0 * 2 ** (pitch / 12)), k
        em_p = plain.push_block(blk, units=units, f0=f0, noise=noise)
        torch.cuda.synchronize()
        assert torch.equal(em, em_p), k
        voiced += int((torch.abs(f0 / 147.0 - 1) < 1e-2).sum())
    assert r.graph_builds == 1 and voiced > 10
