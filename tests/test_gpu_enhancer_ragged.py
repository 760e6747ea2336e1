"""The NSF-HiFiGAN enhancer over RAGGED batches: rows of different length in one padded batch, each row against the CPU oracle
(`oracle.enhancer`, `oracle.resample`) run on that row ALONE at its own length, and exactly 0 after the row's end whatever the
padding holds.  Gates are those of tests/test_gpu_enhancer.py for the same configuration, applied per row.  Shapes are the
smallest that cross the kernels' tile, window and halo boundaries (a 1-frame row is 4 samples at the first stage, under
every halo; 23 frames are 736 samples at the last one, more than one 64-frame window per row)."""
import functools
import json

import numpy as np
import pytest
import torch

import glue_cases as GC
from conftest import rms
from oracle import enhancer as OE
from oracle import resample as OR

pytestmark = pytest.mark.gpu

CONFIGS = {
    "narrow": dict(GC.NSF_CONFIG),
    # the configurations of test_generator_wide_stages / test_generator_shipped_geometry
    "wide": dict(GC.NSF_CONFIG, upsample_rates=[4, 2, 2], upsample_kernel_sizes=[8, 4, 4], upsample_initial_channel=256, num_mels=32),
    "shipped": dict(GC.NSF_CONFIG, upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4],
                    upsample_initial_channel=512, num_mels=128, hop_size=512, n_fft=2048, win_size=2048),
}
SEEDS = {"narrow": GC.NSF_WEIGHT_SEED, "wide": 77, "shipped": 91}
ROWS = {"narrow": [23, 7, 1, 16], "wide": [37, 12, 5], "shipped": [24, 10, 3]}


@functools.lru_cache(maxsize=None)
def _sd(name):
    return GC.nsf_state_dict(CONFIGS[name], seed=SEEDS[name])


@functools.lru_cache(maxsize=None)
def _row(name, L, seed):
    """(mel (1, n_mels, L), f0 (1, L), rand_ini (1, 9), oracle audio (L * upp,)) of one row run alone: computed once."""
    mel, f0, ri = GC.nsf_inputs(CONFIGS[name], L=L, seed=seed)
    want = OE.generator(_sd(name), CONFIGS[name], mel, f0, ri)[0, 0]
    return mel, f0, ri, want


def _rows(name):
    return [_row(name, L, 500 + 13 * j + L) for j, L in enumerate(ROWS[name])]


def _batch(rows, L_max, dev, poison=None):
    """Rows stacked into (B, n_mels, L_max), (B, L_max), (B, 9); the padding holds 0 or `poison`."""
    B, n_mels = len(rows), rows[0][0].shape[1]
    fill = 0.0 if poison is None else poison
    mel = torch.full((B, n_mels, L_max), fill)
    f0 = torch.full((B, L_max), fill)
    for b, (m, f, _, _) in enumerate(rows):
        mel[b, :, :m.shape[-1]] = m[0]
        f0[b, :f.shape[-1]] = f[0]
    return mel.to(dev), f0.to(dev), torch.cat([r[2] for r in rows]).to(dev)


def _generator(name, dev):
    from enhancer import AttrDict, Generator
    return Generator(AttrDict(CONFIGS[name]), _sd(name)).to(dev)


def _upp(name):
    return int(np.prod(CONFIGS[name]["upsample_rates"]))


def _check_rows(name, got, rows, math="fp32_narrow"):
    """Every row of got (B, 1, L_max * upp) against its solo oracle at the configuration's gate; exactly 0 after it."""
    upp = _upp(name)
    for b, (_, _, _, want) in enumerate(rows):
        n = want.numel()
        row = got[b, 0].cpu()
        err = float((row[:n] - want).abs().max())
        print(f"{name} {math} row {b} ({n // upp} frames): max abs error {err:.3e}, |want| max {float(want.abs().max()):.3e}")
        if name == "narrow":
            assert err < 1e-4, (b, err)
        else:
            tol = 3e-4 if math == "split_bf16" else 1e-4
            scale = float(want.abs().max()) if name == "shipped" else 1.0
            assert err < tol * max(1.0, scale), (b, err, scale)
            if name == "shipped":
                assert scale > 1e-3
                assert rms(row[:n] - want) < (3e-5 if math == "split_bf16" else 1e-5) * max(1.0, rms(want) / 0.1), (b, rms(row[:n] - want))
        assert torch.equal(row[n:], torch.zeros_like(row[n:])), (b, "the tail of a row must be exactly 0")


def _set_math(ctx, math):
    import hipddsp
    ctx.set_math(hipddsp.MATH_FP32 if math == "fp32" else hipddsp.MATH_SPLIT_BF16)


def test_generator_narrow_stages(ctx, dev, lib_path):
    """`GC.NSF_CONFIG` (64 / 16 / 4 channel stages... the fused pair kernels and conv_small): n_frames = [23, 7, 1, 16] padded to
    23; zero padding and NaN padding give the same bits."""
    rows, n = _rows("narrow"), ROWS["narrow"]
    gen = _generator("narrow", dev)
    mel, f0, ri = _batch(rows, max(n), dev)
    got = gen(mel, f0, rand_ini=ri, n_frames=n)
    assert got.shape == (4, 1, 23 * _upp("narrow"))
    _check_rows("narrow", got, rows)
    for poison in (float("nan"), 1e30):
        mel_p, f0_p, _ = _batch(rows, max(n), dev, poison=poison)
        assert torch.equal(gen(mel_p, f0_p, rand_ini=ri, n_frames=n), got), poison


@pytest.mark.parametrize("math", ["split_bf16", "fp32"])
@pytest.mark.parametrize("name", ["wide", "shipped"])
def test_generator_wide_and_shipped(ctx, dev, lib_path, name, math):
    """The wide-stage configuration (split-layout activated copies) with n_frames = [37, 12, 5] and the shipped 8-8-2-2-2
    geometry with [24, 10, 3], in both product arithmetics; NaN in the padding changes no bit."""
    rows, n = _rows(name), ROWS[name]
    gen = _generator(name, dev)
    mel, f0, ri = _batch(rows, max(n), dev)
    mel_p, f0_p, _ = _batch(rows, max(n), dev, poison=float("nan"))
    _set_math(ctx, math)
    try:
        got = gen(mel, f0, rand_ini=ri, n_frames=n)
        got_p = gen(mel_p, f0_p, rand_ini=ri, n_frames=n)
    finally:
        _set_math(ctx, "split_bf16")
    _check_rows(name, got, rows, math)
    assert torch.equal(got, got_p)


def test_a_row_does_not_see_its_neighbours(ctx, dev, lib_path):
    """One row in two batches - other neighbours, another slot, another L_max - stays within the gate of its solo oracle."""
    gen = _generator("narrow", dev)
    me = _row("narrow", 7, 901)
    for rows in ([me, _row("narrow", 23, 902), _row("narrow", 2, 903)], [_row("narrow", 16, 904), _row("narrow", 5, 905), me]):
        n = [r[0].shape[-1] for r in rows]
        mel, f0, ri = _batch(rows, max(n), dev, poison=1e30)
        _check_rows("narrow", gen(mel, f0, rand_ini=ri, n_frames=n), rows)


def test_batch_of_one_and_rectangular_batch(ctx, dev, lib_path):
    gen = _generator("narrow", dev)
    mel, f0, ri, _ = _row("narrow", 23, 500 + 23)
    solo = gen(mel.to(dev), f0.to(dev), rand_ini=ri[0])
    assert torch.equal(gen(mel.to(dev), f0.to(dev), rand_ini=ri[0], n_frames=[23]), solo)
    _check_rows("narrow", solo, [_row("narrow", 23, 500 + 23)])
    rows = [_row("narrow", 9, 950 + j) for j in range(3)]            # B = 3, no n_frames: every row is L long
    m, f, r = _batch(rows, 9, dev)
    got = gen(m, f, rand_ini=r)
    assert got.shape == (3, 1, 9 * _upp("narrow"))
    _check_rows("narrow", got, rows)


def test_source_module_per_row(ctx, dev):
    """`ddsp_nsf_source` over a batch: one phase scan per row from the row's own rand_ini, rows [40, 9, 1] at upp 512, against
    `OE.sine_source` of each row alone (5e-6, the gate of test_source_module_against_reference for its long track)."""
    sd = _sd("narrow")
    upp, n = 512, [40, 9, 1]
    g = torch.Generator().manual_seed(21)
    f0 = torch.full((3, 40), float("nan"))
    ri = torch.rand(3, 9, generator=g)
    ri[:, 0] = 0
    want = []
    for b, L in enumerate(n):
        f = 150.0 + 500.0 * torch.rand(1, L, generator=g)
        f0[b, :L] = f[0]
        want.append(OE.sine_source(sd, f, upp, 44100, ri[b:b + 1])[0, :, 0])
    got = ctx.nsf_source(f0.to(dev), ri.to(dev), sd["m_source.l_linear.weight"].reshape(-1).to(dev),
                         sd["m_source.l_linear.bias"].to(dev), upp, 44100, 0.1, ctx.ragged_counts(n)).cpu()
    assert got.shape == (3, 40 * upp)
    for b, L in enumerate(n):
        err = float((got[b, :L * upp] - want[b]).abs().max())
        print(f"source row {b}: {err:.3e}")
        assert err < 5e-6, (b, err)
        assert torch.equal(got[b, L * upp:], torch.zeros(40 * upp - L * upp))


def _stft(h):
    from enhancer import STFT, mel_filterbank
    st = STFT(h["sampling_rate"], h["num_mels"], h["n_fft"], h["win_size"], h["hop_size"], h["fmin"], h["fmax"])
    return st, torch.from_numpy(mel_filterbank(h["sampling_rate"], h["n_fft"], h["num_mels"], h["fmin"], h["fmax"]))


def test_framing_and_log_mel_per_row(dev, lib_path):
    """`STFT.get_mel(n_samples=)` with n_fft 128, hop 32: 4096, 1500 and 70 samples take the reflect branch of the padding rule
    (pad_right = 48 < n), 33 and 20 the constant one (20 was added to the issue's four lengths so that two rows do) - chosen per
    row in one batch; per row against `OE.log_mel`, frame counts included; NaN after each row's samples."""
    h = GC.NSF_CONFIG
    st, basis = _stft(h)
    n = [4096, 1500, 70, 33, 20]
    y = torch.full((len(n), 4100), float("nan"))
    rows = [GC.nsf_audio(T, seed=700 + T) for T in n]
    for b, r in enumerate(rows):
        y[b, :n[b]] = r[0]
    got = st.get_mel(y.to(dev), n_samples=n).cpu()
    wants = [OE.log_mel(r, h, basis) for r in rows]
    assert got.shape == (len(n), h["num_mels"], max(w.shape[-1] for w in wants))
    for b, w in enumerate(wants):
        L = w.shape[-1]
        assert st.frame_count(n[b]) == L, (n[b], L)
        err = float((got[b, :, :L] - w[0]).abs().max())
        print(f"log-mel row {b} ({n[b]} samples, {L} frames): {err:.3e}")
        assert err < 2e-4, (b, err)
        assert torch.equal(got[b, :, L:], torch.zeros_like(got[b, :, L:]))


def _checkpoint(tmp_path, dev, fixed_ri=None):
    from enhancer import Enhancer
    with open(tmp_path / "config.json", "w") as fh:
        json.dump(dict(GC.NSF_CONFIG), fh)
    torch.save({"generator": GC.nsf_state_dict()}, tmp_path / "model")
    if fixed_ri is None:
        return Enhancer("nsf-hifigan", str(tmp_path / "model"), device=dev)

    class Fixed(Enhancer):
        """The harmonics' initial phases are a random draw: pinned, so that two renders can be compared."""

        def enhance(self, *a, **k):
            return super().enhance(*a, rand_ini=fixed_ri, **k)

        def enhance_batch(self, *a, **k):
            return super().enhance_batch(*a, rand_ini=fixed_ri, **k)

    return Fixed("nsf-hifigan", str(tmp_path / "model"), device=dev)


def _cpu_enhance(audio, sr, f0, hop, key, ri):
    """`enhancer.py:24-78` for silence_front = 0 from the oracle's parts (the `cpu_pipeline` of test_enhancer_end_to_end)."""
    h = GC.NSF_CONFIG
    _, basis = _stft(h)
    if key == "auto":
        key = max(0, np.ceil(12 * np.log2(float(torch.max(f0) / 760))))
    fac = 2 ** (-float(key) / 12)
    asr = 100 * int(np.round(44100 / fac / 100))
    rf = 44100 / asr
    a = audio if sr == asr else OR.resample(audio, sr, asr, 128)
    n_frames = int(a.size(-1) // 32 + 1)
    f = f0.squeeze(0).squeeze(-1).numpy().copy() * rf
    t0 = (hop / sr) * np.arange(len(f)) / rf
    t1 = (32 / 44100) * np.arange(n_frames)
    fr = torch.from_numpy(np.interp(t1, t0, f, left=f[0], right=f[-1])).unsqueeze(0).float()
    mel = OE.log_mel(a, h, basis)
    out = OE.generator(GC.nsf_state_dict(), h, mel, fr[:, :mel.size(-1)], ri[None]).reshape(1, -1)
    return OR.resample(out, asr, 44100, 128) if asr != 44100 else out


def test_enhance_batch_end_to_end(dev, lib_path, tmp_path):
    """`Enhancer.enhance_batch` from a checkpoint on disk: rows [4096, 2560, 1024] at hop 512, keys 0, 4 and 'auto' - row 1's f0
    peaks near 1000 Hz (key 5), the others stay at 300 Hz (key 0), so 'auto' splits the batch into two key groups - per row
    against the CPU pipeline of that row alone; n_out equals the solo shapes; NaN past every row's end."""
    enh = _checkpoint(tmp_path, dev)
    ri = torch.tensor([0.0, 0.3, 0.7, 0.1, 0.9, 0.5, 0.2, 0.8, 0.4])
    n, hop = [4096, 2560, 1024], 512
    audio = torch.full((3, 4096), float("nan"))
    f0 = torch.full((3, 8, 1), float("nan"))
    rows = []
    for b, T in enumerate(n):
        a = GC.nsf_audio(T, seed=800 + b)
        fr = T // hop
        track = torch.full((1, fr, 1), 300.0) if b != 1 else (300.0 + 700.0 * torch.sin(torch.arange(fr) / 2.5) ** 2).reshape(1, -1, 1)
        audio[b, :T], f0[b, :fr] = a[0], track[0]
        rows.append((a, track))
    assert float(rows[1][1].max()) > 990
    for key in (0, 4, "auto"):
        got, sr_o, n_out = enh.enhance_batch(audio.to(dev), 44100, f0.to(dev), hop, n, adaptive_key=key, rand_ini=ri)
        assert sr_o == 44100 and got.shape == (3, max(n_out))
        got = got.cpu()
        for b, (a, track) in enumerate(rows):
            want = _cpu_enhance(a, 44100, track, hop, key, ri)
            assert n_out[b] == want.shape[-1], (key, b, n_out[b], want.shape)
            err = float((got[b, :n_out[b]] - want[0]).abs().max())
            print(f"enhance_batch key {key} row {b}: {err:.3e}")
            assert err < 5e-4, (key, b, err)
            assert torch.equal(got[b, n_out[b]:], torch.zeros(got.shape[1] - n_out[b]))
    with pytest.raises(ValueError):
        enh.enhance_batch(audio.to(dev), 44100, f0.to(dev), hop, n, adaptive_key="automatic")


def test_retime_f0_ragged_against_numpy(ctx, dev):
    """`ddsp_retime_f0` with counts, per row against the numpy expression of test_retime_f0_against_numpy: rows with their own
    source and target counts, a single-frame row, targets beyond both ends; ends held at the row's own last frame."""
    rng = np.random.Generator(np.random.PCG64(32))
    for hop, sr, factor, hop_e, sr_e in [(512, 44100, 1.0, 512, 44100), (441, 44100, 1.26, 32, 44100), (160, 16000, 0.7071, 512, 44100)]:
        ns, nd = [173, 87, 1, 40], [173, 120, 5, 700]
        f0 = np.full((4, max(ns)), np.nan, dtype=np.float32)
        for b, n in enumerate(ns):
            f0[b, :n] = rng.uniform(60, 900, n).astype(np.float32)
        got = ctx.retime_f0(torch.from_numpy(f0).to(dev), hop / sr, factor, factor, hop_e / sr_e, max(nd),
                            n_src_dev=ctx.ragged_counts(ns), n_dst_dev=ctx.ragged_counts(nd)).cpu().numpy()
        assert got.shape == (4, max(nd))
        for b, (n, m) in enumerate(zip(ns, nd)):
            vals = f0[b, :n].copy()
            vals *= factor
            t_org = (hop / sr) * np.arange(n) / factor
            want = np.interp((hop_e / sr_e) * np.arange(m), t_org, vals, left=vals[0], right=vals[-1]).astype(np.float32)
            assert np.abs(got[b, :m] - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), (b, np.abs(got[b, :m] - want).max())
            assert not got[b, m:].any()


def test_ragged_generator_replays_bit_identically_under_graph_capture(dev, lib_path):
    """Counts checked and uploaded before the capture (`Generator.counts`): nothing is uploaded or read back inside."""
    import hipddsp
    rows, n = _rows("narrow"), ROWS["narrow"]
    gen = _generator("narrow", dev)
    mel, f0, ri = _batch(rows, max(n), dev, poison=float("nan"))
    gctx = hipddsp.Context(dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s), hipddsp.use_context(gctx):
        counts = gen.counts(n, 4, max(n), dev)
        eager = gen(mel, f0, rand_ini=ri, n_frames=counts)
        eager = gen(mel, f0, rand_ini=ri, n_frames=counts)      # warm-up: scratch arena and weights in place
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = gen(mel, f0, rand_ini=ri, n_frames=counts)
    gctx.freeze()
    torch.cuda.current_stream(dev).wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    _check_rows("narrow", eager, rows)


def test_render_with_the_enhancer_in_ragged_groups(dev, lib_path, tmp_path):
    """`render(..., enhancer_batch_samples=)` against the same `render` with None on a synthetic file of four slices of
    different length, the last two overlapping so that the cross-fade branch runs: file rms error <= 1e-4 (the gate of
    test_convert_batched_with_ragged_units), for a budget that groups two slices and one that groups them otherwise."""
    import infer_offline
    import synthetic
    from ddsp.vocoder import DotDict
    enh = _checkpoint(tmp_path, dev, fixed_ri=torch.tensor([0.0, 0.3, 0.7, 0.1, 0.9, 0.5, 0.2, 0.8, 0.4]))
    lens, starts = [12, 30, 5, 21], [0, 14, 44, 47]
    model, _ = synthetic.build_model("CombSub", seed=7, device=dev)
    whole = synthetic.make_inputs(911, 1, 70, with_noise=False)
    rng = np.random.Generator(np.random.PCG64(912))
    segments = [(s, torch.from_numpy(rng.standard_normal((1, n, 256), dtype=np.float32)).to(dev)) for s, n in zip(starts, lens)]
    args = DotDict({"data": {"block_size": synthetic.HOP, "sampling_rate": synthetic.SR}})
    common = (model, args, segments, whole["f0"].to(dev), whole["volume"].to(dev), whole["spk_id"].to(dev))
    want, sr_w = infer_offline.render(*common, enhancer=enh, noise_seed=3)
    assert sr_w == 44100 and float(np.abs(want).max()) > 1e-3
    for budget in (16000, 40000):
        got, sr_o = infer_offline.render(*common, enhancer=enh, noise_seed=3, enhancer_batch_samples=budget)
        assert sr_o == sr_w and got.shape == want.shape
        err = float(np.sqrt(np.mean((got - want) ** 2)))
        print(f"enhancer_batch_samples {budget}: rms error of the file {err:.3e} (signal rms {float(np.sqrt(np.mean(want ** 2))):.3e})")
        assert err <= 1e-4, (budget, err)
