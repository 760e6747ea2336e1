"""The spectral loss over rows of different length (`RSSLoss.forward(..., n_samples=)`): value and gradient against the
definition written out with torch.stft on every row alone (tests/ragged_defs.py), in fp64.  What follows a row's end is
poisoned, once with garbage and once with NaN."""
import pytest
import torch

from oracle import loss as OL
from ragged_defs import loss_signals, ragged_rss_loss, rel

pytestmark = pytest.mark.gpu
B, T = 3, 6 * 512
N_SAMPLES = [3072, 1500, 290]
SCALES = [256, 300, 777, 2047]     # row 2 has no frame at three of them; row 1 ends inside a frame at every one


def _poisoned(x, n_samples, kind):
    x = x.clone()
    for b, n in enumerate(n_samples):
        x[b, n:] = float("nan") if kind == "nan" else 1e4
    return x


def _last(n, N, hop):
    return 0 if n < N else ((n - N) // hop) * hop + N


@pytest.mark.parametrize("overlap", [0, 0.75])
def test_ragged_loss_value_and_gradient(dev, lib_path, overlap):
    from ddsp.loss import RSSLoss
    xp, xt = loss_signals(5, B, T)
    x64 = xp.double().requires_grad_(True)
    want = ragged_rss_loss(x64, xt.double(), N_SAMPLES, SCALES, overlap=overlap)
    want.backward()
    x32 = xp.clone().requires_grad_(True)
    ragged_rss_loss(x32, xt, N_SAMPLES, SCALES, overlap=overlap).backward()
    cpu_err = rel(x32.grad, x64.grad)
    crit = RSSLoss(256, 2048, 4, overlap=overlap, device=dev)
    got = []
    for kind in ("garbage", "nan"):
        p = _poisoned(xp, N_SAMPLES, kind).to(dev).requires_grad_(True)
        crit.set_scales(SCALES)
        loss = crit(p, _poisoned(xt, N_SAMPLES, kind).to(dev), n_samples=N_SAMPLES)
        loss.backward()
        g = p.grad.cpu()
        e_val, e_grad = abs(float(loss.detach()) - float(want.detach())) / abs(float(want.detach())), rel(g, x64.grad)
        print("overlap", overlap, kind, "value", e_val, "grad", e_grad, "cpu_err", cpu_err)
        assert e_val < 5e-5, (float(loss.detach()), float(want.detach()))
        assert e_grad < max(3 * cpu_err, 4e-3), (e_grad, cpu_err)
        for b, n in enumerate(N_SAMPLES):     # exactly 0 from the end of the row's last whole frame of any scale on
            end = max(_last(n, N, int(N * (1 - overlap))) for N in SCALES)
            assert torch.count_nonzero(g[b, end:]) == 0, (b, end)
        got.append((float(loss.detach()), g))
    assert got[0][0] == got[1][0] and torch.equal(got[0][1], got[1][1])     # the padding is not read


def test_equal_lengths_have_the_bits_of_the_flat_call(ctx, dev):
    xp, xt = loss_signals(6, B, T)
    for hops in (None, [n // 4 for n in SCALES]):
        flat = ctx.rss_loss(xp.to(dev), xt.to(dev), SCALES, want_grad=True, hops=hops)
        full = ctx.rss_loss(xp.to(dev), xt.to(dev), SCALES, want_grad=True, hops=hops, n_samples=[T] * B)
        assert torch.equal(flat[0], full[0]) and torch.equal(flat[1], full[1])


def test_single_scale_and_refusals(dev, lib_path):
    from ddsp.loss import RSSLoss, SSSLoss
    xp, xt = loss_signals(7, B, T)
    want = ragged_rss_loss(xp.double(), xt.double(), N_SAMPLES, [300])
    got = SSSLoss(300)(xt.to(dev), xp.to(dev), n_samples=N_SAMPLES)
    assert abs(float(got) - float(want)) < 5e-5 * float(want)
    # the definition itself, where oracle.loss can express it: rows of one length
    full = ragged_rss_loss(xp.double(), xt.double(), [T] * B, [300, 777])
    assert abs(float(full) - float(OL.rss_loss(xp.double(), xt.double(), [300, 777]))) < 1e-9 * float(full)
    crit = RSSLoss(256, 2048, 2, device=dev)
    crit.set_scales([256, 2047])
    with pytest.raises(ValueError, match="whole frame"):
        crit(xp.to(dev), xt.to(dev), n_samples=[2000, 1500, 290])
    for bad in ([T, T], [T, T, T + 1], [T, 0, T], [T, 2.0, T]):
        with pytest.raises(ValueError):
            crit(xp.to(dev), xt.to(dev), n_samples=bad)
