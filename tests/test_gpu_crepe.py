"""CREPE f0 extractor on the device (ddsp/crepe.py, ddsp.vocoder.F0_Extractor -> ddsp_crepe_activations / ddsp_crepe_decode /
ddsp_f0_postfilter): the network against the fp64 restatement in both product modes, the Viterbi decode against the
full-matrix decode and on a known-answer track, the dither's distribution, the post-filter against the reference's own
(tests/golden/ref_crepe_postfilter.npz), the drop-in with numpy and tensor input, graph capture, the prepared-weight cache and
the refusals."""
import os

import numpy as np
import pytest
import torch

import crepe_cases as CC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

# max |device - fp64| of the sigmoid activations (MI355X: 1.6e-7 in fp32 products, 5.0e-7 in split-bf16)
GATE = {"fp32": 1e-6, "split": 3e-6}


def _model(dev, name="tiny", sd=None):
    from ddsp.crepe import Crepe
    m = Crepe(name)
    m.load_state_dict(CC.fill(name) if sd is None else sd)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def tiny(dev):
    return _model(dev)


def _with_math(ctx, mode):
    import hipddsp
    ctx.set_math(hipddsp.MATH_FP32 if mode == "fp32" else hipddsp.MATH_SPLIT_BF16)


@pytest.mark.parametrize("mode", ["fp32", "split"])
def test_activations_match_the_fp64_restatement(ctx, dev, tiny, mode):
    keep = ctx.math
    _with_math(ctx, mode)
    try:
        errs = {}
        for name in CC.CASES:
            x = CC.audio(name)
            want = CC.activations64(CC.fill("tiny"), x)
            got = tiny.activations(x.to(dev)).cpu().double()
            assert got.shape == want.shape
            errs[name] = float((got - want).abs().max())
        full = _model(dev, "full")
        x = CC.audio("sweep")[:, :1200]   # 16 frames of the 'full' network
        want = CC.activations64(CC.fill("full"), x)
        errs["full"] = float((full.activations(x.to(dev)).cpu().double() - want).abs().max())
    finally:
        ctx.set_math(keep)
    print(mode, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < GATE[mode], errs


def test_decode_returns_the_known_path(ctx, dev):
    path = CC.known_path()
    probs = np.stack([CC.bump_track(len(path), path), CC.bump_track(len(path), path[::-1].copy())])
    p = torch.from_numpy(probs).to(dev)
    f0, pd, bins = ctx.crepe_decode(p, 50, 1100, segment=0, dither=False, want_bins=True)
    bins = bins.cpu().numpy()
    np.testing.assert_array_equal(bins[0], path)
    np.testing.assert_array_equal(bins[1], path[::-1])
    np.testing.assert_allclose(f0.cpu().numpy(), CC.bin_to_hz(bins), rtol=2e-7)
    np.testing.assert_array_equal(pd.cpu().numpy(), np.take_along_axis(probs, bins[..., None], 2)[..., 0])


def test_decode_equals_the_full_matrix_decode(ctx, dev, tiny):
    """Same activations in, same bins out - wherever no decision on the restatement's path is closer than 1e-6 (an ulp of an
    emission can flip such a decision) - with the reference's pieces of 512 frames."""
    rng = np.random.default_rng(3)
    tracks = [tiny.activations(CC.audio("sweep").to(dev))[0].cpu().numpy(),
              rng.uniform(0, 1, (700, 360)).astype(np.float32)]
    compared = 0
    for probs in tracks:
        _, _, bins = ctx.crepe_decode(torch.from_numpy(probs)[None].to(dev), 65, 800, segment=512, want_bins=True)
        bins = bins[0].cpu().numpy()
        for s in range(0, len(probs), 512):
            want, margins = CC.viterbi_naive(CC.emissions(probs[s:s + 512], 65, 800))
            if margins[0] <= 1e-6:
                continue
            small = np.nonzero(margins[1:] <= 1e-6)[0]
            t0 = small[-1] + 1 if len(small) else 0          # frames from the last close decision on
            np.testing.assert_array_equal(bins[s + t0: s + len(want)], want[t0:])
            compared += len(want) - t0
    assert compared > 400


def test_dither_is_triangular_and_seeded(ctx, dev):
    path = CC.known_path()
    probs = torch.from_numpy(np.stack([CC.bump_track(len(path), np.roll(path, k)) for k in range(40)])).to(dev)   # 12640
    f_plain, _ = ctx.crepe_decode(probs, 50, 1100, dither=False)
    f_a, _ = ctx.crepe_decode(probs, 50, 1100, dither_seed=1234, dither=True)
    f_b, _ = ctx.crepe_decode(probs, 50, 1100, dither_seed=1234, dither=True)
    f_c, _ = ctx.crepe_decode(probs, 50, 1100, dither_seed=99, dither=True)
    assert torch.equal(f_a, f_b) and not torch.equal(f_a, f_c)
    assert torch.equal(f_plain, ctx.crepe_decode(probs, 50, 1100, dither=False)[0])
    cents = lambda f: 1200 * np.log2(f.cpu().double().numpy() / 10)   # noqa: E731
    off = (cents(f_a) - cents(f_plain)).ravel()
    assert off.size >= 10_000
    assert off.min() > -20 and off.max() < 20
    assert abs(off.mean()) < 0.3
    assert abs(off.var() / (20 ** 2 / 6) - 1) < 0.05


def test_postfilter_matches_the_reference(ctx, dev):
    fix = np.load(os.path.join(GOLDEN, "ref_crepe_postfilter.npz"))
    for i in range(len(fix["sr"])):
        f0 = torch.from_numpy(fix[f"f0_in_{i}"])[None].to(dev)
        pd = torch.from_numpy(fix[f"pd_in_{i}"])[None].to(dev)
        got = ctx.f0_postfilter(f0, pd, int(fix["sr"][i]), float(fix["hop"][i]), int(fix["n_frames"][i]),
                                int(fix["start_frame"][i]), 0.05, bool(fix["uv_interp"][i]), float(fix["f0_min"][i]))
        got = got[0].cpu().numpy()
        want = fix[f"out_{i}"]
        ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, (i, int(ulp.max()), int((ulp > 0).sum()))


def _sweep(sr, seconds, f=150.0, seed=0):
    t = np.arange(int(sr * seconds)) / sr
    rng = np.random.default_rng(seed)
    return (0.3 * np.sin(2 * np.pi * f * t * (1 + 0.3 * t)) + 0.01 * rng.standard_normal(len(t))).astype(np.float32)


def test_extract_numpy_tensor_and_batch(dev, tiny):
    from ddsp.vocoder import F0_Extractor
    ex = F0_Extractor("crepe", 44100, 512, 65, 800, crepe_ckpt=tiny, device=dev)
    a, b = _sweep(44100, 1.2, 150, 1), _sweep(44100, 1.2, 220, 2)
    n_frames = len(a) // 512 + 1
    out = ex.extract(a, uv_interp=True, silence_front=0.3, dither=False)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (n_frames,)
    assert np.all(out >= 65) and np.all(np.isfinite(out))
    t = ex.extract(torch.from_numpy(a).to(dev), uv_interp=True, silence_front=0.3, dither=False)
    assert t.is_cuda and t.shape == (n_frames,)
    np.testing.assert_array_equal(t.cpu().numpy(), out)
    both = ex.extract(torch.from_numpy(np.stack([a, b])).to(dev), dither=False)
    assert both.shape == (2, n_frames)
    np.testing.assert_array_equal(both[0].cpu().numpy(), ex.extract(a, dither=False))
    np.testing.assert_array_equal(both[1].cpu().numpy(), ex.extract(b, dither=False))
    # dithered by default, within a bin of the undithered track
    d = ex.extract(a, seed=5)
    np.testing.assert_array_equal(d, ex.extract(a, seed=5))
    plain = ex.extract(a, dither=False)
    assert not np.array_equal(d, plain)
    ratio = d[plain > 0] / plain[plain > 0]
    assert ratio.size > 0 and np.all(np.abs(np.log2(ratio) * 1200) < 20.5)


def test_extract_at_48k_with_a_fractional_hop(dev, tiny):
    from ddsp.vocoder import F0_Extractor
    hop = 512 * 48000 / 44100
    ex = F0_Extractor("crepe", 48000, hop, 50, 1100, crepe_ckpt=tiny, device=dev)
    a = _sweep(48000, 4.5, 180, 3)
    out = ex.extract(a, uv_interp=True, silence_front=1.47, dither=False)
    assert out.shape == (int(len(a) // hop) + 1,)
    assert out.dtype == np.float32 and np.all(np.isfinite(out)) and np.all(out >= 50)


def test_graph_replay_equals_eager(dev, tiny):
    import hipddsp
    from ddsp.vocoder import F0_Extractor
    ex = F0_Extractor("crepe", 44100, 512, 65, 800, crepe_ckpt=tiny, device=dev)
    x = torch.from_numpy(_sweep(44100, 1.5, 200, 4)).to(dev)
    gctx = hipddsp.Context(dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s), hipddsp.use_context(gctx):
        eager = ex.extract(x, uv_interp=True, silence_front=0.2, dither=False)
        eager = ex.extract(x, uv_interp=True, silence_front=0.2, dither=False)   # warm-up: arena at size
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = ex.extract(x, uv_interp=True, silence_front=0.2, dither=False)
    gctx.freeze()
    torch.cuda.current_stream(dev).wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_prepared_weights_follow_writes(dev):
    m = _model(dev)
    x = CC.audio("sweep").to(dev)
    first = m.activations(x)
    assert torch.equal(m.activations(x), first)   # cached
    sd = {k: (v * 1.1 if k.endswith("conv2.weight") else v) for k, v in CC.fill("tiny").items()}
    m.load_state_dict(sd)
    fresh = _model(dev, sd=sd)
    after = m.activations(x)
    assert not torch.equal(after, first)
    assert torch.equal(after, fresh.activations(x))
    with torch.no_grad():
        m.conv4_BN.running_var.mul_(2.0)
        fresh.conv4_BN.running_var.mul_(2.0)
    assert torch.equal(m.activations(x), _model(dev, sd={k: v.cpu() for k, v in fresh.state_dict().items()}).activations(x))
    # a write torch does not count needs rebind()
    m.conv5.bias.data.add_(0.5)
    m.rebind()
    ref = _model(dev, sd={k: v.cpu() for k, v in m.state_dict().items()})
    assert torch.equal(m.activations(x), ref.activations(x))


def test_refusals(dev, tiny):
    from ddsp.vocoder import F0_Extractor
    ex = F0_Extractor("crepe", 44100, 512, crepe_ckpt=tiny, device=dev)
    with pytest.raises(RuntimeError):
        ex.extract(torch.zeros(44100))                      # a CPU tensor
    with pytest.raises(ValueError):
        ex.extract(np.zeros(300, dtype=np.float32))         # 109 samples at 16 kHz: 2 CREPE frames
    ex.extract(np.zeros(441, dtype=np.float32))             # 160 samples: 3 frames, the shortest accepted
    with pytest.raises(RuntimeError):
        F0_Extractor("crepe", 44100, 512, crepe_ckpt=tiny, device="cpu")
