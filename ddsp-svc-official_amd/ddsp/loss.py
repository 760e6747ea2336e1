"""Drop-in for the reference's `ddsp/loss.py` (`SSSLoss`, `RSSLoss`), evaluated by libddsp_amd (value AND
gradient w.r.t. the prediction come from hand-written kernels; no CPU fallback).

`RSSLoss(fft_min, fft_max, n_scale, alpha=1.0, overlap=0, eps=1e-7, device='cuda')(x_pred, x_true)` draws
`n_scale` integers in [fft_min, fft_max) with `torch.randint` per call exactly like the reference
(`ddsp/loss.py:39`), so seeding torch reproduces the reference's sequence of scales; `set_scales` pins the next
draw (tests, and data-parallel ranks that must share one draw - SURVEY 8e).  `overlap` sets the hop as the reference
does, `int(n_fft * (1 - overlap))` (`ddsp/loss.py:13`); its callers use 0 (`train.py:48`).

Additive: `forward(..., n_samples=None)` on both classes - rows of DIFFERENT LENGTH inside the padded (B, T) signals (a sequence
of B ints or a CPU integer tensor (B,), 1 <= n_samples[b] <= T).  At scale N row b has F_b = (n_samples[b] - N) // hop + 1
STFT frames, or none if it is shorter than N.  The convergence term is the mean of ||S_t - S_p||_F / ||S_t + S_p||_F over the
rows that have a frame, each norm over the row's own frames; the log term is the mean of |ln S_t - ln S_p| over the
sum_b F_b * (N // 2 + 1) cells that exist.  Nothing at or after sample (F_b - 1) * hop + N of a row is read into arithmetic
(the kernels select), the gradient is exactly 0 from there on, and with every count equal to T value and gradient have the bits
of the call without counts.  A scale at which no row has a frame raises ValueError before anything is launched.

Additive: `forward(..., n_samples=, global_n_samples=)` on both classes - the rows are ONE RANK'S SHARE of a global batch
(data-parallel training on ragged shards).  `global_n_samples` is a sequence of ints (or a CPU integer tensor) with the sample
counts of every rank's rows, the local rows somewhere among them; every entry is positive and at least one global row has a
frame at every drawn scale (ValueError before anything is launched otherwise).  The two denominators - the rows with a frame
and the cells that exist - are taken over the global rows, the sums over the local ones: the value is this rank's share of the
global loss and the gradient the gradient of that share.  Shares summed over the ranks give the one-process loss; gradients
summed over the ranks, WITHOUT a division by the number of ranks, its gradient.  A rank whose own rows have no frame at some
scale is allowed; its share at that scale is 0.  With `global_n_samples` equal to `n_samples` value and gradient have the bits
of the call without it.  A rectangular local batch in a ragged global batch passes `n_samples=[T] * B`.

Additive: `RSSLoss.rows(x_pred, x_true, n_samples)` -> (B,), one loss per row and no gradient (validation, where every
utterance counts once): row b is what `forward` returns for `x[b:b+1, :n_samples[b]]` alone, both terms over the row's own
cells, from the same kernels up to the per-row statistics.  Every row needs a frame at every drawn scale (ValueError before
anything is launched otherwise).
"""
import torch
import torch.nn as nn

import hipddsp


class _SpectralLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_pred, x_true, n_ffts, alpha, eps, overlap=0, n_samples=None, global_n_samples=None):
        c = hipddsp.context_for(x_pred.device)
        need = x_pred.requires_grad
        hops = None if overlap == 0 else [_hop(n, overlap) for n in n_ffts]
        loss, grad = c.rss_loss(x_pred, x_true, n_ffts, alpha, eps, want_grad=need, hops=hops, n_samples=n_samples,
                                global_n_samples=global_n_samples)
        ctx.grad = grad
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        grad = ctx.grad
        ctx.grad = None
        return (grad * g if grad is not None else None), None, None, None, None, None, None, None


def _hop(n_fft, overlap):
    """The reference's hop (`ddsp/loss.py:13`), in Python floats like there."""
    return int(n_fft * (1 - overlap))


def _check(x_pred, x_true, overlap, n_samples=None):
    """Host checks of the arguments -> `n_samples` as a checked list (None: rows of one length)."""
    if not 0 <= overlap < 1:
        raise ValueError("overlap must lie in [0, 1)")
    if n_samples is None:
        return None
    if x_pred.dim() != 2:
        raise ValueError("n_samples= needs (B, T) signals")
    return hipddsp.check_n_samples(n_samples, x_pred.shape[0], x_pred.shape[1])


def _check_global(n_samples, global_n_samples):
    """-> `global_n_samples` as a checked list (None: the local rows are the whole batch)."""
    if global_n_samples is None:
        return None
    if n_samples is None:
        raise ValueError("global_n_samples= needs n_samples= (a rectangular local batch passes n_samples=[T] * B)")
    return hipddsp.check_global_n_samples(global_n_samples, n_samples)


def _need_device(x_pred):
    if not x_pred.is_cuda:
        raise RuntimeError("the spectral loss runs on a HIP device only (no CPU fallback)")


class SSSLoss(nn.Module):
    """Single-scale spectral loss (reference `ddsp/loss.py:7-25`); call order is (x_true, x_pred) as there."""

    def __init__(self, n_fft=111, alpha=1.0, overlap=0, eps=1e-7):
        super().__init__()
        self.n_fft, self.alpha, self.overlap, self.eps = int(n_fft), alpha, overlap, eps

    def forward(self, x_true, x_pred, n_samples=None, global_n_samples=None):
        """`n_samples`: rows of different length; `global_n_samples`: the rows are one rank's share of a global batch
        (module docstring)."""
        n_samples = _check(x_pred, x_true, self.overlap, n_samples)
        global_n_samples = _check_global(n_samples, global_n_samples)
        if n_samples is not None:
            hipddsp.check_loss_scales(n_samples if global_n_samples is None else global_n_samples, [self.n_fft])
        _need_device(x_pred)
        return _SpectralLossFn.apply(x_pred, x_true.to(x_pred.dtype), [self.n_fft], self.alpha, self.eps, self.overlap,
                                     n_samples, global_n_samples)


class RSSLoss(nn.Module):
    """Random-scale spectral loss (reference `ddsp/loss.py:28-43`)."""

    def __init__(self, fft_min, fft_max, n_scale, alpha=1.0, overlap=0, eps=1e-7, device="cuda"):
        super().__init__()
        self.fft_min, self.fft_max, self.n_scale = fft_min, fft_max, n_scale
        self.alpha, self.overlap, self.eps = alpha, overlap, eps
        self._pinned = None
        self.last_scales = None

    def set_scales(self, n_ffts):
        """Use these scales for the next call instead of drawing (one-shot)."""
        self._pinned = [int(n) for n in n_ffts]

    def _draw(self):
        """The scales of one call: the pinned draw (used up) or `torch.randint` as the reference draws (`ddsp/loss.py:39`)."""
        if self._pinned is not None:
            n_ffts, self._pinned = self._pinned, None
        else:
            n_ffts = [int(v) for v in torch.randint(self.fft_min, self.fft_max, (self.n_scale,))]
        self.last_scales = n_ffts
        return n_ffts

    def forward(self, x_pred, x_true, n_samples=None, global_n_samples=None):
        """`n_samples`: rows of different length; `global_n_samples`: the rows are one rank's share of a global batch
        (module docstring).  The scales are drawn (and a pinned draw is used up) before the counts are checked against
        them."""
        n_samples = _check(x_pred, x_true, self.overlap, n_samples)
        global_n_samples = _check_global(n_samples, global_n_samples)
        if n_samples is None:
            _need_device(x_pred)
        n_ffts = self._draw()
        if n_samples is not None:
            hipddsp.check_loss_scales(n_samples if global_n_samples is None else global_n_samples, n_ffts)
            _need_device(x_pred)
        # cached training audio may be fp16 (reference data_loaders.py:81-83): promote the target
        return _SpectralLossFn.apply(x_pred, x_true.to(torch.float32), n_ffts, self.alpha, self.eps, self.overlap, n_samples,
                                     global_n_samples)

    def rows(self, x_pred, x_true, n_samples):
        """One loss per row, (B,), without a gradient (module docstring).  The scales are drawn, or a pinned draw is used up,
        exactly as in `forward`."""
        if n_samples is None:
            raise ValueError("rows: n_samples is required (the rows' lengths)")
        n_samples = _check(x_pred, x_true, self.overlap, n_samples)
        n_ffts = self._draw()
        for b, n in enumerate(n_samples):
            if n < max(n_ffts):
                raise ValueError(f"n_samples[{b}] = {n}: the row holds no whole frame at scale n_fft = {max(n_ffts)}")
        _need_device(x_pred)
        hops = None if self.overlap == 0 else [_hop(n, self.overlap) for n in n_ffts]
        loss, _ = hipddsp.context_for(x_pred.device).rss_loss(x_pred, x_true.to(torch.float32), n_ffts, self.alpha, self.eps,
                                                              hops=hops, n_samples=n_samples, rows=True)
        return loss
