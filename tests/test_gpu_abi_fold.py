"""One C entry point per operation (ABI 8) on the device: the argument pairings that no symbol reached before the fold are
refused with a message that names the surviving symbol and leave the context usable; the folded optimiser entry runs the
arithmetic of the symbols it absorbed; S rows of the real-time glue are the bits of S one-row calls."""
import ctypes

import numpy as np
import pytest
import torch

import hipddsp
from hipddsp import _ptr

pytestmark = pytest.mark.gpu
B = 2


def _i32(dev, *vals):
    return torch.tensor(vals, dtype=torch.int32, device=dev)


def _refusals(dev):
    """(surviving symbol, arguments after (ctx, stream)) of every newly refused pairing; nothing here reaches a kernel."""
    f = lambda *shape: torch.zeros(*shape, device=dev)
    n2 = _i32(dev, 5, 3)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    probs, f0, pd, out6 = f(B, 6, 360), f(B, 6), f(B, 6), f(B, 6)
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    x = f(B, 64)
    loss, ffts = f(1), ints(16)
    units, cw = f(B, 4, 8), hipddsp.CrepeWeights()
    decode_tail = (50.0, 1000.0, 0, 0)
    post = lambda nc, start, no: ("ddsp_f0_postfilter", (_ptr(f0), _ptr(pd), B, 6, nc, 16000, 80.0, 6, start, no, 0.05, 0, 65.0, _ptr(out6)))
    rss = lambda ns, ns_dev, gns, ng: ("ddsp_rss_loss", (_ptr(x), _ptr(x), B, 64, ns, ns_dev, gns, ng, ffts, None, 1, 1.0, 1e-7,
                                                         _ptr(loss), None))
    return [
        # seed_dev together with n_frames
        ("ddsp_crepe_decode", (_ptr(probs), B, 6, _ptr(n2), *decode_tail, _ptr(seed), 0, _ptr(f0), _ptr(pd), None)),
        # start_frame != 0 together with counts
        post(_ptr(n2), 1, _ptr(n2)),
        ("ddsp_f0_ac", (_ptr(x), B, 64, _ptr(n2), 16000, 80.0, 750.0, 1100.0, 2, 1, 0, _ptr(f(B, 2)), None)),
        # one pointer of a pair without the other
        post(_ptr(n2), 0, None), post(None, 0, _ptr(n2)),
        rss(ints(64, 32), None, None, 0), rss(None, _ptr(_i32(dev, 64, 32)), None, 0),
        ("ddsp_align_units", (_ptr(units), B, 4, 8, 6, 1.0, _ptr(n2), None, _ptr(f(B, 6, 8)))),
        ("ddsp_align_units", (_ptr(units), B, 4, 8, 6, 1.0, None, _ptr(n2), _ptr(f(B, 6, 8)))),
        ("ddsp_retime_f0", (_ptr(f0), B, 6, _ptr(n2), 1.0, 1.0, 1.0, 1.0, 6, None, _ptr(out6))),
        ("ddsp_retime_f0", (_ptr(f0), B, 6, None, 1.0, 1.0, 1.0, 1.0, 6, _ptr(n2), _ptr(out6))),
        ("ddsp_crepe_activations", (ctypes.byref(cw), _ptr(x), B, 64, _ptr(n2), None, 2, 80, _ptr(f(B, 1, 360)))),
        ("ddsp_crepe_activations", (ctypes.byref(cw), _ptr(x), B, 64, None, _ptr(_i32(dev, 0, 1, 2)), 2, 80, _ptr(f(B, 1, 360)))),
        # a batch without counts where the kernel finds its row by them
        ("ddsp_retime_f0", (_ptr(f0), B, 6, None, 1.0, 1.0, 1.0, 1.0, 6, None, _ptr(out6))),
        # global counts without local counts
        rss(None, None, ints(64, 32, 64), 3),
    ]


def test_new_pairings_are_refused_and_the_context_lives_on(dev, lib_path):
    ctx = hipddsp.Context(dev)
    cases = _refusals(dev)
    assert len(cases) == 15
    for name, args in cases:
        with pytest.raises(ValueError, match=name + r"\b(?!_)") as e:
            ctx.call(name, *args)
        assert str(e.value).startswith(name + ": " + name + ": "), str(e.value)     # the library's own text, not ctypes'
    torch.cuda.synchronize()
    ctx.poll_error()
    x = torch.arange(12, device=dev, dtype=torch.float32).reshape(1, 4, 3)
    up = ctx.upsample(x, 2)
    assert up.shape == (1, 8, 3) and torch.equal(up[0, ::2], x[0])


def _adamw_state(dev, n=1000):
    g = torch.Generator().manual_seed(8)
    p, grad, m = (torch.randn(n, generator=g).to(dev) for _ in range(3))
    v = torch.rand(n, generator=g).to(dev)
    return p, grad, m, v


HYPER = dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=3)


def test_adamw_multi_with_unit_scale_is_the_single_tensor_step(dev, lib_path):
    ctx = hipddsp.Context(dev)
    p0, grad, m0, v0 = _adamw_state(dev)
    p1, m1, v1 = p0.clone(), m0.clone(), v0.clone()
    ctx.adamw_step(p0, grad, m0, v0, **HYPER)
    ctx.adamw_step_multi([p1], [grad], [m1], [v1], **HYPER, grad_scale=1.0)
    torch.cuda.synchronize()
    assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1)


def test_adamw_multi_with_half_scale_is_the_step_on_the_halved_gradient(dev, lib_path):
    ctx = hipddsp.Context(dev)
    p0, grad, m0, v0 = _adamw_state(dev)
    p1, m1, v1 = p0.clone(), m0.clone(), v0.clone()
    ctx.adamw_step_multi([p0], [grad * 0.5], [m0], [v0], **HYPER, grad_scale=1.0)      # (a power of two: the product is exact)
    keep = grad.clone()
    ctx.adamw_step_multi([p1], [grad], [m1], [v1], **HYPER, grad_scale=0.5)
    torch.cuda.synchronize()
    assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1)
    assert torch.equal(grad, keep)                                                     # the gradients are not written
    with pytest.raises(ValueError, match="finite"):
        ctx.call("ddsp_adamw_step_multi", 0, None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, float("nan"))


def test_two_rows_of_the_stream_glue_are_two_one_row_calls(dev, lib_path):
    """ddsp_stream_push / ddsp_sola / ddsp_phase_vocoder with S = 2 against two S = 1 calls, bit for bit (the shapes of
    test_sola_stream_against_oracle and the GUI's 1764-sample cross-fade of test_phase_vocoder_matches_reference)."""
    from frontend_cases import pv_inputs
    ctx = hipddsp.Context(dev)
    block, xfade, search, delay, n = 8820, 1764, 441, 882, 44544
    rng = np.random.Generator(np.random.PCG64(31))
    t = np.arange(n) / 44100
    audio = torch.from_numpy(np.stack([0.3 * np.sin(2 * np.pi * f * t + p) + 0.01 * rng.standard_normal(n)
                                       for f, p in ((196.0, 0.0), (233.1, 1.3))]).astype(np.float32)).to(dev)
    start = n - block - xfade - search - delay                                         # the buffers: the rows' own audio at lags 100, 300
    buf = torch.stack([audio[s, start + lag:start + lag + xfade] for s, lag in ((0, 100), (1, 300))]).contiguous()
    rows = [ctx.sola(audio[s], b, block, xfade, search, delay) + (b,) for s, b in ((0, buf[0].clone()), (1, buf[1].clone()))]
    both = buf.clone()
    emitted, shift = ctx.sola(audio, both, block, xfade, search, delay)
    for s, (em, sh, b) in enumerate(rows):
        assert torch.equal(emitted[s], em) and int(shift[s]) == int(sh[0]) and torch.equal(both[s], b), s
    assert shift.tolist() == [100, 300]                                                # each row found its own arg-max

    blocks = torch.from_numpy(rng.standard_normal((2, block)).astype(np.float32)).to(dev)
    solo = [ctx.stream_push_(audio[s].clone(), blocks[s].clone()) for s in range(2)]
    win = ctx.stream_push_(audio.clone(), blocks)
    for s in range(2):
        assert torch.equal(win[s], solo[s]) and torch.equal(win[s, -block:], blocks[s]) and torch.equal(win[s, :-block], audio[s, block:])

    a, b, fo, fi = (v.to(dev) for v in pv_inputs(0))
    a2, b2 = torch.stack([a, b.flip(0)]), torch.stack([b, a.flip(0)])
    out = ctx.phase_vocoder(a2, b2, fo, fi)
    for s in range(2):
        assert torch.equal(out[s], ctx.phase_vocoder(a2[s], b2[s], fo, fi)), s
    torch.cuda.synchronize()
    ctx.poll_error()
