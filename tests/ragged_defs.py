"""What the ragged-training tests share (not a test module): the spectral loss over rows of different length, written from
its definition with torch.stft (oracle.loss has no per-row lengths), and the signals of the loss tests."""
import numpy as np
import torch


def ragged_rss_loss(x_pred, x_true, n_samples, n_ffts, alpha=1.0, eps=1e-7, overlap=0.0):
    """Row b has F_b = (n_b - N) // hop + 1 frames at scale N (none when n_b < N).  Per scale: the mean over the rows that
    have a frame of ||S_t - S_p||_F / ||S_t + S_p||_F (each norm over the row's own frames) + alpha * the mean of
    |ln S_t - ln S_p| over the cells that exist; then the mean over the scales.  S = |STFT| / sqrt(sum w^2) + eps with a
    periodic Hann window, center=False (torchaudio Spectrogram(power=1, normalized=True) as oracle.loss restates it)."""
    total = 0.0
    for N in n_ffts:
        hop = int(N * (1 - overlap))
        w = torch.hann_window(N, periodic=True, dtype=x_pred.dtype)
        norm = w.pow(2).sum().sqrt()
        conv, l1, cells, rows = 0.0, 0.0, 0, 0
        for b, n in enumerate(n_samples):
            if n < N:
                continue
            F = (n - N) // hop + 1
            end = (F - 1) * hop + N
            S = [torch.stft(x[b, :end], N, hop, N, window=w, center=False, return_complex=True).abs() / norm + eps
                 for x in (x_true, x_pred)]
            assert S[0].shape == (N // 2 + 1, F)
            conv = conv + torch.linalg.norm(S[0] - S[1]) / torch.linalg.norm(S[0] + S[1])
            l1 = l1 + (S[0].log() - S[1].log()).abs().sum()
            cells += F * (N // 2 + 1)
            rows += 1
        assert rows > 0
        total = total + conv / rows + alpha * l1 / cells
    return total / len(n_ffts)


def loss_signals(seed, B, T):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(T) / 44100
    xt = 0.1 * rng.standard_normal((B, T)) + 0.2 * np.sin(2 * np.pi * 220 * t)[None]
    xp = 0.1 * rng.standard_normal((B, T)) + 0.15 * np.sin(2 * np.pi * 233 * t + 0.3)[None]
    return torch.from_numpy(xp.astype(np.float32)), torch.from_numpy(xt.astype(np.float32))


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
