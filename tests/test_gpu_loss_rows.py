"""`RSSLoss.rows` (ddsp_rss_loss_rows): one loss per row of a ragged batch, against the same loss on every row rendered and
scored alone, against the per-file losses of the reference's validation run (tests/golden/ref_solver.npz), and against
`forward` where the two must agree.

Tolerance of a loss VALUE: 2e-5 relative, the one tests/test_gpu_loss.py applies to the value against its reference fixture.
Bit equality with the solo call does NOT fall out of the shared statistics: `loss_stats_kernel` cuts a row into 16 chunks of
the PADDED row's cells, so row b's fp64 partial sums are formed in another order inside the batch than alone."""
import numpy as np
import pytest
import torch

import solver_cases as SC

pytestmark = pytest.mark.gpu
TOL = 2e-5


@pytest.fixture(scope="module")
def case(dev):
    z = SC.load()
    n = [int(k) * SC.HOP for k in z["frames"]]
    T = max(n)
    xp, xt = torch.zeros(len(n), T), torch.zeros(len(n), T)
    for i, k in enumerate(n):
        xp[i, :k] = torch.from_numpy(z[f"pred_{i}"])
        xt[i, :k] = torch.from_numpy(z[f"audio_{i}"][:k])
    return {"xp": xp.to(dev), "xt": xt.to(dev), "n": n, "scales": [int(s) for s in z["scales"]], "losses": z["losses"]}


def _crit(dev, overlap=0):
    from ddsp.loss import RSSLoss
    return RSSLoss(SC.FFT_MIN, SC.FFT_MAX, SC.N_SCALE, overlap=overlap, device=dev)


def _rows(crit, case, xp=None, xt=None, n=None):
    crit.set_scales(case["scales"])
    out = crit.rows(case["xp"] if xp is None else xp, case["xt"] if xt is None else xt, case["n"] if n is None else n)
    assert out.shape == (len(case["n"]),) and out.dtype == torch.float32 and crit._pinned is None      # the pinned draw is used up
    return out


def test_rows_against_the_reference_run(dev, lib_path, case):
    got = _rows(_crit(dev), case).cpu().double().numpy()
    print("rows", got, "fixture", case["losses"], "rel", np.abs(got / case["losses"] - 1))
    assert np.all(np.abs(got - case["losses"]) < TOL * case["losses"])


@pytest.mark.parametrize("overlap", [0, 0.5])
def test_rows_against_every_row_alone(dev, lib_path, case, overlap):
    crit = _crit(dev, overlap)
    got = _rows(crit, case).cpu().double().numpy()
    for b, k in enumerate(case["n"]):
        crit.set_scales(case["scales"])
        solo = float(crit(case["xp"][b:b + 1, :k].contiguous(), case["xt"][b:b + 1, :k].contiguous()))
        print("overlap", overlap, "row", b, got[b], solo, abs(got[b] / solo - 1))
        assert abs(got[b] - solo) < TOL * solo, (b, got[b], solo)


@pytest.mark.parametrize("decoy", [1e4, float("nan")])
def test_what_follows_a_row_changes_nothing(dev, lib_path, case, decoy):
    crit = _crit(dev)
    clean = _rows(crit, case)
    xp, xt = case["xp"].clone(), case["xt"].clone()
    for b, k in enumerate(case["n"]):
        xp[b, k:] = decoy
        xt[b, k:] = decoy
    assert torch.equal(_rows(crit, case, xp, xt), clean)


def test_equal_counts_mean_of_rows_is_forward(dev, lib_path, case):
    """With all counts equal the mean of `rows()` is `forward()`.  The convergence term has that structure always: `forward`
    takes the mean over the rows of the same per-row ratio.  The log term coincides ONLY for equal counts: `forward` divides
    the batch's sum of |ln S_t - ln S_p| by the batch's number of cells, a mean over the rows weighted by their cell counts,
    while `rows()` divides row b's sum by row b's cells - the two are equal exactly when every row has the same number.
    What is left is fp32 rounding: either side adds its n_scale terms in fp32 (at most n_scale * eps / 2 each, relative to
    the value, all terms being positive), and `forward` rounds its fp64 batch mean once more per scale where the mean below is
    taken in fp64: 2 * n_scale * eps bounds the difference."""
    crit = _crit(dev)
    k = case["n"][1]                                   # 9 frames: one frame at 2047, 18 at 256
    xp, xt = case["xp"][:, :k].contiguous(), case["xt"][:, :k].contiguous()
    n = [k] * xp.shape[0]
    rows = _rows(crit, case, xp, xt, n).cpu().double().numpy()
    crit.set_scales(case["scales"])
    flat = float(crit(xp, xt, n_samples=n))
    crit.set_scales(case["scales"])
    assert float(crit(xp, xt)) == flat                 # (the ragged call with full counts has the flat call's bits)
    print("mean of rows", rows.mean(), "forward", flat)
    assert abs(rows.mean() - flat) <= 2 * len(case["scales"]) * np.finfo(np.float32).eps * flat


def test_a_row_without_a_frame_is_refused_before_any_launch(ctx, dev, case):
    crit = _crit(dev)
    n = list(case["n"])
    n[2] = 2046                                        # no frame at 2047
    crit.set_scales(case["scales"])
    with pytest.raises(ValueError, match=r"n_samples\[2\]"):
        crit.rows(case["xp"], case["xt"], n)
    with pytest.raises(ValueError, match="ddsp_rss_loss_rows"):             # the library's own check of the host counts
        ctx.rss_loss(case["xp"], case["xt"], case["scales"], n_samples=n, rows=True)
    with pytest.raises(ValueError):
        ctx.rss_loss(case["xp"], case["xt"], case["scales"], rows=True)     # rows need counts
    with pytest.raises(ValueError):
        crit.rows(case["xp"], case["xt"], None)
