"""Ragged volume (`Volume_Extractor.extract(audio (B,T), n_samples=)` -> ddsp_volume_extract with n_samples): every row against the
restatement behind tests/test_gpu_frontend.py (oracle.frontend.volume_extract) applied to THAT ROW ALONE, at that test's
bound of 2e-6 relative; exact zeros after a row's frames; the padding (NaN, or noise) is never seen."""
import numpy as np
import pytest
import torch

from oracle import frontend as OF

pytestmark = pytest.mark.gpu

HOP, T = 512, 5000
N = [257, 511, 512, 513, 1024, 5000]     # the shortest legal row, both sides of one hop, an exact multiple, the full row


def test_volume_of_every_row_as_if_alone(ctx, dev):
    from ddsp.vocoder import Volume_Extractor
    rng = np.random.default_rng(31)
    audio = rng.uniform(-1, 1, (len(N), T)).astype(np.float32)
    ve = Volume_Extractor(HOP, device=dev)
    outs = []
    for fill in (np.nan, None):
        x = audio.copy()
        for b, n in enumerate(N):
            x[b, n:] = fill if fill is not None else rng.uniform(-1, 1, T - n)
        outs.append(ve.extract(torch.from_numpy(x).to(dev), n_samples=N))
    assert torch.equal(outs[0], outs[1]), "the padding's content reached the result"
    got = outs[0].cpu().numpy()
    assert outs[0].is_cuda and got.shape == (len(N), T // HOP + 1) and np.all(np.isfinite(got))
    for b, n in enumerate(N):
        want = OF.volume_extract(audio[b, :n], HOP)
        assert want.shape == (n // HOP + 1,)
        assert np.allclose(got[b, :len(want)], want, rtol=2e-6, atol=0), (b, np.abs(got[b, :len(want)] - want).max())
        assert not got[b, len(want):].any(), f"row {b}: the tail is not 0"
    # the full row equals the rectangular call, and a tensor of counts is accepted
    assert torch.equal(outs[0][5], ve.extract(torch.from_numpy(audio[5]).to(dev)))
    assert torch.equal(ve.extract(torch.from_numpy(audio).to(dev), n_samples=torch.tensor(N)), ctx.volume_extract(
        torch.from_numpy(audio).to(dev), HOP, n_samples=N))


def test_refusals(dev):
    from ddsp.vocoder import Volume_Extractor
    ve = Volume_Extractor(HOP, device=dev)
    x = torch.zeros(2, T, device=dev)
    for bad in ([256, T], [0, T], [T + 1, T], [T], torch.tensor([T, T], device=dev)):
        with pytest.raises(ValueError):
            ve.extract(x, n_samples=bad)
    with pytest.raises(ValueError):
        Volume_Extractor(557.29, device=dev).extract(x, n_samples=[T, T])     # a fractional hop has no ragged form
    with pytest.raises(ValueError):
        ve.extract(x[0], n_samples=[T])                                        # a ragged batch is (B, T)
