"""Drop-in for the reference's `enhancer.py` (`Enhancer`, `NsfHifiGAN`) and the inference half of `nsf_hifigan/models.py`
(`load_model`, `Generator` with `SineGen` / `SourceModuleHnNSF`) and `nsf_hifigan/nvSTFT.py` (`STFT.get_mel`), executed by
libddsp_amd on the device (no CPU path).

    Enhancer(enhancer_type, enhancer_ckpt, device).enhance(audio (1,T), sample_rate, f0 (1,Fr,1), hop_size,
                                                           adaptive_key=0 | 'auto', silence_front=0) -> (audio (1,T'), sr)
    Enhancer.enhance_batch(audio (B,T), sample_rate, f0 (B,Fr,1), hop_size, n_samples, adaptive_key=0 | 'auto')
                                                           -> (audio (B,T'_max), sr, n_out): rows of different length in one
    padded batch, every row as if enhanced alone at its own length and 0 after it (`Generator.forward(..., n_frames=)`,
    `STFT.get_mel(..., n_samples=)`, `NsfHifiGAN.forward(..., n_samples=)` are the same contract one level down).

Checkpoints are read with `torch.load(weights_only=True)` (`{'generator': state_dict}` next to a `config.json`, as
`nsf_hifigan/models.py:24-39` expects); weight-normed layers (`weight_g`, `weight_v`) are folded at load time like the
reference's `remove_weight_norm()`.  Two third-party boundaries are restated from their published algorithms and are
PARITY UNPINNED (neither package is in the image): librosa's Slaney mel filter bank (`nvSTFT.py:85`) and torchaudio's
resampler (`enhancer.py:50-53,69-73`, see resample.py).  Everything else is pinned by fixtures generated from the
reference's own `nsf_hifigan/models.py` (tests/golden/make_golden.py tier f).
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import hipddsp
from ddsp.hubert import RaggedCounts
from resample import Resample

LRELU_SLOPE = 0.1


class AttrDict(dict):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.__dict__ = self


# ---- constant tables ------------------------------------------------------------------------------------------------------
def mel_filterbank(sr, n_fft, n_mels, fmin, fmax):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) with its defaults (Slaney scale, Slaney area normalisation),
    restated from librosa's published algorithm -> (n_mels, n_fft//2 + 1) float32."""
    def hz_to_mel(f):
        f = np.asanyarray(f, dtype=np.float64)
        f_sp = 200.0 / 3
        mels = f / f_sp
        min_log_hz = 1000.0
        min_log_mel = min_log_hz / f_sp
        logstep = np.log(6.4) / 27.0
        return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-12) / min_log_hz) / logstep, mels)

    def mel_to_hz(m):
        m = np.asanyarray(m, dtype=np.float64)
        f_sp = 200.0 / 3
        min_log_hz = 1000.0
        min_log_mel = min_log_hz / f_sp
        logstep = np.log(6.4) / 27.0
        return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)

    fmax = float(sr) / 2 if fmax is None else fmax
    fftfreqs = np.linspace(0, float(sr) / 2, 1 + n_fft // 2)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    weights = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    return (weights * enorm[:, None]).astype(np.float32)


class STFT:
    """`nsf_hifigan/nvSTFT.py:52-119` for keyshift = 0, speed = 1: reflect padding, Hann(periodic) window, magnitude with the
    1e-9 floor, mel projection, log of the clamped value.  `get_mel(y (1,T)) -> (1, n_mels, frames)`;
    `get_mel(y (B,T), n_samples=)` -> (B, n_mels, L_max): a ragged batch, row b framed and padded as its own n_samples[b]
    samples would be alone (reflect or zeros, chosen per row), 0 in the frames after its own `frame_count(n_samples[b])`."""

    def __init__(self, sr=22050, n_mels=80, n_fft=1024, win_size=1024, hop_length=256, fmin=20, fmax=11025, clip_val=1e-5):
        if win_size != n_fft:
            raise ValueError("only win_size == n_fft (every shipped NSF-HiFiGAN config) is built")
        self.target_sr, self.n_mels, self.n_fft, self.win_size, self.hop_length = sr, n_mels, n_fft, win_size, hop_length
        self.fmin, self.fmax, self.clip_val = fmin, fmax, clip_val
        self._tables = {}

    def _device_tables(self, device):
        key = str(device)
        if key not in self._tables:
            n, bins = self.n_fft, self.n_fft // 2 + 1
            ldm = (bins + 3) & ~3
            i = torch.arange(n, dtype=torch.float64)
            f = torch.arange(bins, dtype=torch.float64)
            ang = 2 * np.pi * torch.outer(f, i) / n
            win = torch.hann_window(n, dtype=torch.float64)
            tab = torch.zeros(2 * ldm, n, dtype=torch.float64)
            tab[0:2 * bins:2] = torch.cos(ang) * win
            tab[1:2 * bins:2] = -torch.sin(ang) * win
            mel = torch.zeros(self.n_mels, ldm)
            mel[:, :bins] = torch.from_numpy(mel_filterbank(self.target_sr, n, self.n_mels, self.fmin, self.fmax))
            self._tables[key] = (tab.float().to(device).contiguous(), mel.to(device).contiguous())
        return self._tables[key]

    def frame_count(self, n_samples):
        """Frames `get_mel` gives for a signal of n_samples (host integers: nvSTFT.py:88-98 pads, torch.stft frames)."""
        n, hop = self.n_fft, self.hop_length
        pad_left = (n - hop) // 2
        pad_right = max((n - hop + 1) // 2, n - int(n_samples) - pad_left)
        return (int(n_samples) + pad_left + pad_right - n) // hop + 1

    def get_mel(self, y, keyshift=0, speed=1, center=False, n_samples=None, n_frames=None):
        """`n_samples` / `n_frames` as two `RaggedCounts`: a ragged batch whose counts live on the device only (the rows'
        samples, and their `frame_count` with `n_frames.T` the padded frame axis) - nothing is checked on the host or
        uploaded, so the call can be captured."""
        if keyshift != 0 or speed != 1 or center:
            raise ValueError("only keyshift = 0, speed = 1, center = False (how the Enhancer calls it) is built")
        if y.dim() != 2:
            raise ValueError("STFT.get_mel: y must be (B, T)")
        if isinstance(n_samples, RaggedCounts) or isinstance(n_frames, RaggedCounts):
            if not (isinstance(n_samples, RaggedCounts) and isinstance(n_frames, RaggedCounts)):
                raise ValueError("STFT.get_mel: device counts need both n_samples and n_frames as RaggedCounts")
            if n_samples.T != y.shape[1] or len(n_samples.values) != y.shape[0] or len(n_frames.values) != y.shape[0]:
                raise ValueError("STFT.get_mel: these RaggedCounts were made for another batch shape")
            if not y.is_cuda:
                raise RuntimeError("STFT.get_mel runs on a HIP device only (no CPU fallback)")
            return self._get_mel_batch(y, None, dev_counts=(n_samples.dev, n_frames.dev, n_frames.T))
        if n_frames is not None:
            raise ValueError("STFT.get_mel: n_frames goes with n_samples as RaggedCounts")
        vals = None if n_samples is None else hipddsp.check_n_samples(n_samples, y.shape[0], y.shape[1])
        if not y.is_cuda:
            raise RuntimeError("STFT.get_mel runs on a HIP device only (no CPU fallback)")
        if y.shape[0] != 1 or vals is not None:
            return self._get_mel_batch(y, vals)
        n, hop = self.n_fft, self.hop_length
        pad_left = (n - hop) // 2
        pad_right = max((n - hop + 1) // 2, n - y.size(-1) - pad_left)
        mode = "reflect" if pad_right < y.size(-1) else "constant"
        yp = F.pad(y.unsqueeze(1), (pad_left, pad_right), mode=mode).squeeze(1)           # (memory movement only)
        # (torch framing on purpose: the tests hold `stft_frames`, the device framing of the other shapes, against this path)
        frames = yp[0].unfold(0, n, hop).contiguous()                                      # (frames, n_fft)
        tab, mel = self._device_tables(y.device)
        out = hipddsp.context_for(y.device).log_mel(frames, tab, mel, self.clip_val)      # (frames, n_mels)
        return out.t().unsqueeze(0)

    def _get_mel_batch(self, y, vals, dev_counts=None):
        """Rows of different length (vals: checked counts, None = every row whole): framing on the device with the padding
        rule chosen per row, then the spectral half on B * L_max rows.  dev_counts = (samples (B,), frames (B,), L): the counts
        as device tensors only."""
        B, T = y.shape
        c = hipddsp.context_for(y.device)
        if dev_counts is not None:
            n_dev, f_dev, L = dev_counts
            frames = c.stft_frames(y, n_dev, self.n_fft, self.hop_length, L)
            tab, mel = self._device_tables(y.device)
            out = c.log_mel(frames.reshape(B * L, self.n_fft), tab, mel, self.clip_val).reshape(B, L, self.n_mels)
            return c.ragged_frames(out, f_dev, hold=False).transpose(1, 2)
        frames_of = [self.frame_count(v) for v in (vals if vals is not None else [T] * B)]
        L = max(frames_of)
        n_dev = None if vals is None else c.ragged_counts(vals)
        frames = c.stft_frames(y, n_dev, self.n_fft, self.hop_length, L)
        tab, mel = self._device_tables(y.device)
        out = c.log_mel(frames.reshape(B * L, self.n_fft), tab, mel, self.clip_val).reshape(B, L, self.n_mels)
        if vals is not None:          # log-mel of an empty frame is log(clip), not 0
            out = c.ragged_frames(out, c.ragged_counts(frames_of), hold=False)
        return out.transpose(1, 2)


# ---- the generator -------------------------------------------------------------------------------------------------------------
def _fold_weight_norm(sd, prefix):
    """weight of a layer stored either plain or as (weight_g, weight_v) of torch.nn.utils.weight_norm (dim 0)."""
    if prefix + ".weight" in sd:
        return sd[prefix + ".weight"].float()
    g, v = sd[prefix + ".weight_g"].float(), sd[prefix + ".weight_v"].float()
    return v * (g / v.norm(dim=(1, 2), keepdim=True))


def _pack_conv(w):
    """Conv1d weight (Cout, Cin, k) -> (Cout, k*Cin), column = tap*Cin + ci (the GEMM's implicit-im2col order)."""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()


def _split_or_none(w_packed):
    """The packed weight in the split operand layout (hipddsp.presplit), or None where its rows are not whole groups of 8."""
    return hipddsp.presplit(w_packed) if w_packed.shape[1] % 8 == 0 else None


def _pack_conv_transpose(w, stride):
    """ConvTranspose1d weight (Cin, Cout, k), padding (k - stride)//2 -> the 3-tap convolution that produces all `stride`
    output phases at once: (stride*Cout, 3*Cin), row = r*Cout + co, column = tap*Cin + ci, value W[ci][co][r + p - (tap-1)*u]."""
    Cin, Cout, k = w.shape
    u, p = stride, (k - stride) // 2
    if (k - stride) % 2 or k < u:
        raise ValueError("unsupported ConvTranspose1d geometry")
    out = torch.zeros(u * Cout, 3 * Cin, dtype=w.dtype)
    covered = torch.zeros(u, k, dtype=torch.bool)
    for r in range(u):
        for tap in range(3):
            kk = r + p - (tap - 1) * u
            if 0 <= kk < k:
                out[r * Cout:(r + 1) * Cout, tap * Cin:(tap + 1) * Cin] = w[:, :, kk].t()
                covered[r, kk] = True
    # every kernel tap that reaches output phase r must have been placed
    for r in range(u):
        for kk in range(k):
            if (kk - r - p) % u == 0 and not covered[r, kk]:
                raise ValueError("ConvTranspose1d kernel too long for the 3-tap form")
    return out.contiguous()


class Generator(torch.nn.Module):
    """`nsf_hifigan/models.py:219-276` (inference).  Built from the reference's state dict; `forward(x (B, n_mels, L), f0 (B, L))
    -> (B, 1, L * prod(upsample_rates))`.  `rand_ini` (9,) or (B, 9) injects the harmonics' random initial phases (the
    reference draws them with torch.rand; element 0 is forced to 0 like there).
    `n_frames` (a sequence of B ints or a CPU integer tensor, 1 <= n_frames[b] <= L; checked on the host, uploaded once): a
    RAGGED batch - row b comes out, over its first n_frames[b] * upp samples, as the row run alone at its own length, and
    exactly 0 after them, whatever x and f0 hold past n_frames[b].  None: every row is L long.  `Generator.counts` checks and
    uploads ahead of the call (inside a HIP graph capture nothing may be uploaded): pass what it returns as `n_frames`."""

    def __init__(self, h, state_dict=None):
        super().__init__()
        self.h = h
        self.num_kernels = len(h.resblock_kernel_sizes)
        self.num_upsamples = len(h.upsample_rates)
        self.upp = int(np.prod(h.upsample_rates))
        if str(h.resblock) != "1":
            raise ValueError("only ResBlock1 generators (every shipped NSF-HiFiGAN config) are built")
        if len(h.resblock_kernel_sizes) > 3:
            raise ValueError("at most three residual blocks per stage")
        self._packed = None
        if state_dict is not None:
            self.load_reference_state(state_dict)

    def load_reference_state(self, sd):
        h = self.h
        P = {}
        P["lin_w"] = sd["m_source.l_linear.weight"].float().reshape(-1).contiguous()
        P["lin_b"] = sd["m_source.l_linear.bias"].float().reshape(-1).contiguous()
        if P["lin_w"].numel() != 9:
            raise ValueError("the source module merges 9 harmonics")
        w = _fold_weight_norm(sd, "conv_pre")
        P["pre_w"], P["pre_b"], P["pre_k"] = _pack_conv(w), sd["conv_pre.bias"].float().contiguous(), w.shape[2]
        P["pre_ws"] = _split_or_none(P["pre_w"])
        ch = h.upsample_initial_channel
        P["ups"], P["noise"], P["res"] = [], [], []
        for i, (u, k) in enumerate(zip(h.upsample_rates, h.upsample_kernel_sizes)):
            w = _fold_weight_norm(sd, f"ups.{i}")
            if w.shape[0] != ch // (2 ** i) or w.shape[1] != ch // (2 ** (i + 1)):
                raise ValueError("upsampling layer shape does not match the config")
            b = sd[f"ups.{i}.bias"].float()
            w_up = _pack_conv_transpose(w, u)
            P["ups"].append((w_up, _split_or_none(w_up), b.repeat(u).contiguous(), u, w.shape[1]))
            nw = sd[f"noise_convs.{i}.weight"].float()
            if i + 1 < len(h.upsample_rates):
                s = int(np.prod(h.upsample_rates[i + 1:]))
                geo = (2 * s, s, s // 2)
            else:
                geo = (1, 1, 0)
            if nw.shape[2] != geo[0]:
                raise ValueError("noise convolution shape does not match the config")
            P["noise"].append((nw.reshape(nw.shape[0], -1).contiguous(), sd[f"noise_convs.{i}.bias"].float().contiguous(), geo))
            blocks = []
            for j, (k, dils) in enumerate(zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes)):
                n = i * self.num_kernels + j
                convs = []
                for t, d in enumerate(dils):
                    w1 = _fold_weight_norm(sd, f"resblocks.{n}.convs1.{t}")
                    w2 = _fold_weight_norm(sd, f"resblocks.{n}.convs2.{t}")
                    p1, p2 = _pack_conv(w1), _pack_conv(w2)
                    convs.append((p1, _split_or_none(p1), sd[f"resblocks.{n}.convs1.{t}.bias"].float().contiguous(), int(d),
                                  p2, _split_or_none(p2), sd[f"resblocks.{n}.convs2.{t}.bias"].float().contiguous(), int(k)))
                blocks.append(convs)
            P["res"].append(blocks)
        w = _fold_weight_norm(sd, "conv_post")
        P["post_w"] = w[0].t().contiguous().reshape(-1)          # (k, C) tap-major
        P["post_b"], P["post_k"] = sd["conv_post.bias"].float().contiguous(), w.shape[2]
        self._packed = P
        self._dev = None

    def to(self, device=None, *a, **k):
        self._target = torch.device(device) if device is not None else None
        return self

    def _on(self, device):
        if self._dev is None or self._dev[0] != device:
            def mv(x):
                if torch.is_tensor(x):
                    return x.to(device)
                if isinstance(x, (list, tuple)):
                    return type(x)(mv(y) for y in x)
                return x
            self._dev = (device, {k: mv(v) for k, v in self._packed.items()})
        return self._dev[1]

    @staticmethod
    def counts(n_frames, B, L, device):
        """`n_frames` of a ragged (B, n_mels, L) batch, checked on the host and uploaded once -> `RaggedCounts`."""
        vals = hipddsp.check_n_frames(n_frames, B, L)
        return RaggedCounts(vals, L, hipddsp.context_for(device).ragged_counts(vals))

    @torch.no_grad()
    def forward(self, x, f0, rand_ini=None, n_frames=None):
        if x.dim() != 3:
            raise ValueError("Generator: x must be (B, n_mels, L)")
        B, n_mels, L = x.shape
        if isinstance(n_frames, RaggedCounts):
            if len(n_frames.values) != B or n_frames.T != L or n_frames.dev.device != x.device:
                raise ValueError("Generator: these RaggedCounts were made for another batch shape or device")
            n_dev = n_frames.dev
        elif n_frames is not None:
            n_frames = hipddsp.check_n_frames(n_frames, B, L)          # ValueError before anything is launched
        if not x.is_cuda:
            raise RuntimeError("the NSF-HiFiGAN generator runs on a HIP device only (no CPU fallback)")
        P = self._on(x.device)
        c = hipddsp.context_for(x.device)
        if n_frames is None:
            n_dev = None
        elif not isinstance(n_frames, RaggedCounts):
            n_dev = c.ragged_counts(n_frames)
        # B rows flattened on the time axis, (B * T, C); `rows(scale)` tells a call where each row ends at the current rate
        # (n_dev None: every row whole)
        def rows(scale):
            return (B, n_dev, scale)

        f0 = f0.reshape(B, -1)[:, :L].contiguous().float()
        if rand_ini is None:
            rand_ini = torch.rand(B, 9)
        rand_ini = rand_ini.float()
        rand_ini = (rand_ini.reshape(1, 9).expand(B, 9) if rand_ini.numel() == 9 else rand_ini.reshape(B, 9)).clone()
        rand_ini[:, 0] = 0
        rand_ini = rand_ini.to(x.device)
        sr = int(self.h.sampling_rate)
        src = c.nsf_source(f0, rand_ini, P["lin_w"], P["lin_b"], self.upp, sr, 0.1, n_dev)                  # (B, L * upp)
        # Every convolution below reads leaky_relu(., 0.1) of its producer's result (models.py:60-62, 251): the producers
        # write that activated copy themselves (`act_slope`), next to the raw result where a residual path or the stage mean
        # needs it, so that the consumers take their input as it is (in_slope = 1) and run on the LDS-DMA GEMM.  With
        # split-bf16 products (the context's default) the activated copies of the 64-channel-multiple stages are written in the
        # split operand layout and the weights were converted at load: those convolutions split nothing in their loops.
        use_split = c.math == hipddsp.MATH_SPLIT_BF16

        def can_split(cin, cout):
            """A convolution can write its activated output split when it runs on the DMA kernel itself (Cin % 32 == 0) and
            its output rows are whole 64-column tiles."""
            return use_split and cin % 32 == 0 and cout % 64 == 0

        ch0 = int(self.h.upsample_initial_channel)
        act_s = can_split(n_mels, ch0)               # is the current activated tensor in the split layout?
        xin = x.transpose(1, 2).contiguous()         # (B, L, n_mels)
        if n_dev is not None:                        # what a convolution reads is 0 past the row's end: the mel may hold anything
            xin = c.ragged_frames(xin.float(), n_dev, hold=False)
        _, cur_act = c.conv1d(xin.reshape(B * L, n_mels), P["pre_w"], P["pre_b"], P["pre_k"], 1, 1.0, want_out=False,
                              act_slope=LRELU_SLOPE, w_split=P["pre_ws"] if act_s else None, act_split=act_s,
                              rows=rows(1))          # (B * L, C0)
        T, cin = L, ch0
        cur = None
        for i in range(self.num_upsamples):
            w_up, w_up_s, b_up, u, cout = P["ups"][i]
            nw, nb, (nk, ns, npad) = P["noise"][i]
            T_out = T * u
            x_source = c.nsf_noise_conv(src, nw, nb, nk, ns, npad, T_out)                          # (B * T_out, cout)
            s_out = can_split(cin, cout)
            # a narrow stage whose residual pairs run fused (x in, x out, activations on load: csrc/nsf.hip, conv_pair*) needs no
            # activated copies at all
            fused = all(c.conv1d_pair_supported(cout, k, d) for convs in P["res"][i] for (_, _, _, d, _, _, _, k) in convs)
            # (the (B * T, u * cout) result is the (B * T_out, cout) output, u samples of one row per line: masked per INPUT row)
            up, up_act = c.conv1d(cur_act, w_up, b_up, 3, 1, 1.0, residual=x_source.reshape(B * T, u * cout),
                                  act_slope=None if fused else LRELU_SLOPE,
                                  w_split=w_up_s if (act_s or s_out) else None, x_split=act_s, act_split=s_out,
                                  rows=rows(T // L)), None
            if not fused:
                up, up_act = up
            cur, cur_act = up.reshape(B * T_out, cout), None if fused else up_act.reshape(B * T_out, cout)
            T = T_out
            here = rows(T // L)                       # every convolution of this stage runs at this rate
            outs = []
            s = s_out                                 # inside a stage every convolution is cout -> cout
            ws_ok = use_split and cout % 32 == 0      # pre-split weights alone still save the weight half of the in-loop split
            for convs in P["res"][i]:
                xr, xr_act = cur, cur_act
                for t, (w1, w1s, b1, d, w2, w2s, b2, k) in enumerate(convs):
                    if fused:
                        xr, _ = c.conv1d_pair(xr, w1, b1, w2, b2, k, d, LRELU_SLOPE, rows=here)
                        continue
                    _, xt_act = c.conv1d(xr_act, w1, b1, k, d, 1.0, want_out=False, act_slope=LRELU_SLOPE,
                                         w_split=w1s if ws_ok else None, x_split=s, act_split=s, rows=here)
                    if t + 1 < len(convs):
                        xr, xr_act = c.conv1d(xt_act, w2, b2, k, 1, 1.0, residual=xr, act_slope=LRELU_SLOPE,
                                              w_split=w2s if ws_ok else None, x_split=s, act_split=s, rows=here)
                    else:
                        xr = c.conv1d(xt_act, w2, b2, k, 1, 1.0, residual=xr, w_split=w2s if ws_ok else None, x_split=s,
                                      rows=here)
                outs.append(xr)
            if i + 1 < self.num_upsamples:
                act_s = use_split and cout % 64 == 0   # the mean kernel writes either layout
                _, cur_act = c.nsf_mean(outs, want_out=False, act_slope=LRELU_SLOPE, act_split=act_s)
            else:
                cur = c.nsf_mean(outs)
            cin = cout
        # (the stage means need no counts: the mean of tensors that are 0 past a row's end is 0 there)
        audio = c.nsf_post(cur, P["post_w"], P["post_b"], P["post_k"], 0.01, rows(self.upp))
        return audio.reshape(B, 1, -1)

    __call__ = forward


def load_model(model_path, device="cuda"):
    """`nsf_hifigan/models.py:24-39`: config.json beside the checkpoint, `cp_dict['generator']`."""
    with open(os.path.join(os.path.split(model_path)[0], "config.json")) as fh:
        h = AttrDict(json.load(fh))
    cp = torch.load(model_path, map_location="cpu", weights_only=True)
    gen = Generator(h, cp["generator"])
    gen.to(device)
    return gen, h


class NsfHifiGAN(torch.nn.Module):
    """`enhancer.py:81-101`."""

    def __init__(self, model_path, device=None):
        super().__init__()
        self.device = "cuda" if device is None else device
        print("| Load HifiGAN: ", model_path)
        self.model, self.h = load_model(model_path, device=self.device)
        self._stft = None

    def sample_rate(self):
        return self.h.sampling_rate

    def hop_size(self):
        return self.h.hop_size

    def stft(self):
        h = self.h
        if self._stft is None:
            self._stft = STFT(h.sampling_rate, h.num_mels, h.n_fft, h.win_size, h.hop_size, h.fmin, h.fmax)
        return self._stft

    def forward(self, audio, f0, rand_ini=None, n_samples=None):
        """audio (B, T), f0 (B, frames) -> (enhanced (B, T'_max), sample rate).  `n_samples`: a ragged batch, row b being its
        first n_samples[b] samples; it comes out as the row enhanced alone in its first `frame_count(n_samples[b]) * hop`
        samples and 0 after them.  f0 must cover every row's own frames; what it holds past them is not read."""
        stft = self.stft()
        vals = None if n_samples is None else hipddsp.check_n_samples(n_samples, audio.shape[0], audio.shape[-1])
        with torch.no_grad():
            mel = stft.get_mel(audio, n_samples=vals)
            n_frames = None if vals is None else [stft.frame_count(v) for v in vals]
            enhanced = self.model(mel, f0.reshape(f0.shape[0], -1)[:, :mel.size(-1)], rand_ini=rand_ini, n_frames=n_frames)
            return enhanced.reshape(audio.shape[0], -1), self.h.sampling_rate


class KeyedPlan:
    """What `Enhancer.enhance_keyed` needs besides the audio, for one geometry (T samples and Fr f0 frames per row at
    `sample_rate` / `hop_size`, `silence_front`, keys 0..max_key), built once.
    Host part (the constructor; no device is touched): `rates[k]`, the working rate of key k, and `lengths[k]`, the five integers
    of `Enhancer.batch_lengths` for the cut row at that rate; `widths`, the five column maxima that size every buffer; the
    front cut and the front pad.  Device part (`on(device)`, once per device): the lengths, the key thresholds and the
    re-timing scalars as tensors, and the two resampler plans (into the working rates and back) with their tap tables.
    DIVERGENCE: the reference's 'auto' key is unbounded; here keys above `max_key` are clamped to it, because the set of
    working rates - tap tables, buffer sizes - has to be finite."""

    def __init__(self, enhancer, T, Fr, sample_rate, hop_size, silence_front=0, max_key=12):
        if isinstance(max_key, bool) or not isinstance(max_key, int) or not 0 <= max_key <= 12:
            raise ValueError(f"KeyedPlan: max_key must be an int in 0..12, got {max_key!r}")
        self.T, self.Fr, self.sample_rate, self.hop_size = int(T), int(Fr), int(sample_rate), hop_size
        self.silence_front, self.max_key = silence_front, max_key
        self.sr_e, self.hop_e = int(enhancer.enhancer_sample_rate), int(enhancer.enhancer_hop_size)
        self.cut_frames, self.cut_samples, cut_seconds = enhancer._front_cut(silence_front, sample_rate, hop_size)
        self.front_pad = int(np.round(self.sr_e * cut_seconds)) if self.cut_frames > 0 else 0
        self.T_cut, self.Fr_cut = self.T - self.cut_samples, self.Fr - self.cut_frames
        if self.T_cut < 1 or self.Fr_cut < 1:
            raise ValueError(f"KeyedPlan: silence_front = {silence_front} leaves no audio or no f0 frame of the row")
        self.rates, self.pitch_scales = [], []
        for k in range(max_key + 1):
            rate, scale, _ = enhancer._working_rate(k, None)
            for a, b in ((self.sample_rate, rate), (rate, self.sr_e)):
                g = int(np.gcd(a, b)) if a >= 1 and b >= 1 else 0
                if g < 1 or a // g >= 65536 or b // g >= 65536:
                    raise ValueError(f"KeyedPlan: the resampler cannot pair {a} Hz with {b} Hz (key {k})")
            self.rates.append(rate)
            self.pitch_scales.append(scale)
        self.lengths = [tuple(enhancer.batch_lengths(self.T_cut, self.sample_rate, r)) for r in self.rates]
        self.widths = tuple(max(row[i] for row in self.lengths) for i in range(5))
        self.pairs_in = [(self.sample_rate, r) for r in self.rates]
        self.pairs_out = [(r, self.sr_e) for r in self.rates]
        self.n_out = [row[4] + self.front_pad for row in self.lengths]        # per key, the front pad included
        self._dev = {}

    def on(self, device):
        """The device part, built on first use for `device` (uploads and tap tables: before any capture)."""
        dev = torch.device(device)
        key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
        if key not in self._dev:
            c = hipddsp.context_for(dev)
            d = AttrDict()
            d.lengths = torch.tensor(self.lengths, dtype=torch.int32).to(dev)                     # (max_key + 1, 5)
            d.thresholds = torch.from_numpy(hipddsp.key_thresholds(self.max_key)).to(dev)
            d.div = torch.tensor(self.pitch_scales, dtype=torch.float64).to(dev)
            d.scale = torch.tensor(self.pitch_scales, dtype=torch.float32).to(dev)
            d.rs_in = c.resample_plan(self.pairs_in, 128)
            d.rs_out = c.resample_plan(self.pairs_out, 128)
            if d.rs_in.length(self.T_cut) != self.widths[0] or d.rs_out.length(self.widths[3]) < self.widths[4]:
                raise RuntimeError("KeyedPlan: the resampler plans disagree with batch_lengths")
            self._dev[key] = d
        return self._dev[key]


class Enhancer:
    """`enhancer.py:9-78`, same constructor and `enhance` signature."""

    def __init__(self, enhancer_type, enhancer_ckpt, device=None):
        self.device = "cuda" if device is None else device
        if enhancer_type == "nsf-hifigan":
            self.enhancer = NsfHifiGAN(enhancer_ckpt, device=self.device)
        else:
            raise ValueError(f" [x] Unknown enhancer: {enhancer_type}")
        self.resample_kernel = {}
        self.enhancer_sample_rate = self.enhancer.sample_rate()
        self.enhancer_hop_size = self.enhancer.hop_size()

    # -- the three decisions of `enhance` that do not touch audio ------------------------------------------------------
    @staticmethod
    def _front_cut(silence_front, sample_rate, hop_size):
        """(frames, samples, seconds) of the silent front that is skipped and padded back (enhancer.py:27-31,76-77)."""
        frames = int(silence_front * sample_rate / hop_size)
        seconds = frames * hop_size / sample_rate
        return frames, int(np.round(seconds * sample_rate)), seconds

    def _working_rate(self, adaptive_key, f0):
        """The rate the generator is run at for a key shift of `adaptive_key` semitones (enhancer.py:33-43): the audio is
        treated as if sampled at 100 * round(sr_e * 2^(key/12) / 100) Hz, which moves every pitch down by the key.
        'auto' picks the smallest non-negative key that brings the highest f0 under 760 Hz - that one number decides
        tensor LENGTHS, so it is the single value read back from the device (a max over a few hundred frames)."""
        if isinstance(adaptive_key, str):
            if adaptive_key != "auto":
                raise ValueError(f"adaptive_key must be a number or 'auto', got {adaptive_key!r}")
            adaptive_key = max(0, np.ceil(12 * np.log2(float(torch.max(f0) / 760))))
            print("auto_adaptive_key: " + str(int(adaptive_key)))
        shrink = 2 ** (-float(adaptive_key) / 12)
        rate = 100 * int(np.round(self.enhancer_sample_rate / shrink / 100))
        return rate, self.enhancer_sample_rate / rate, shrink

    def _resampled(self, x, rate_in, rate_out):
        if rate_in == rate_out:
            return x
        pair = (int(rate_in), int(rate_out))
        if pair not in self.resample_kernel:
            self.resample_kernel[pair] = Resample(rate_in, rate_out, lowpass_filter_width=128)
        return self.resample_kernel[pair](x)

    def enhance(self, audio, sample_rate, f0, hop_size, adaptive_key=0, silence_front=0, rand_ini=None):
        """audio (1,T), f0 (1,n_frames,1) -> (enhanced (1,T'), enhancer sample rate); reference `enhancer.py:24-78`.
        Device only: the f0 track is re-timed to the generator's frames by `ddsp_retime_f0`, nothing is copied to the host
        (with adaptive_key='auto' one scalar - the highest f0 - is read back, see `_working_rate`)."""
        cut_frames, cut_samples, cut_seconds = self._front_cut(silence_front, sample_rate, hop_size)
        audio, f0 = audio[:, cut_samples:], f0[:, cut_frames:, :]
        work_rate, pitch_scale, shrink = self._working_rate(adaptive_key, f0)
        audio_res = self._resampled(audio, sample_rate, work_rate)
        n_frames = int(audio_res.size(-1) // self.enhancer_hop_size + 1)
        # f0 of frame i of the generator = the track (scaled by pitch_scale, its time axis divided by it) at i * hop_e / sr_e
        f0_res = hipddsp.context_for(audio.device).retime_f0(f0, hop_size / sample_rate, pitch_scale, pitch_scale,
                                                               self.enhancer_hop_size / self.enhancer_sample_rate, n_frames)[None]
        enhanced, sr_e = self.enhancer(audio_res, f0_res, rand_ini=rand_ini)
        if shrink != 0:
            enhanced = self._resampled(enhanced, work_rate, sr_e)
        if cut_frames > 0:
            enhanced = F.pad(enhanced, (int(np.round(sr_e * cut_seconds)), 0))
        return enhanced, sr_e

    # -- rows with a key of their own in one batch: nothing asks the host --------------------------------------------------
    def keyed_plan(self, T, Fr, sample_rate, hop_size, silence_front=0, max_key=12):
        return KeyedPlan(self, T, Fr, sample_rate, hop_size, silence_front, max_key)

    @staticmethod
    def check_key_request(adaptive_key, max_key, what="adaptive_key"):
        """'auto' -> -1, a whole number in 0..max_key -> that int; anything else raises ValueError (a host check)."""
        if isinstance(adaptive_key, str):
            if adaptive_key != "auto":
                raise ValueError(f"{what} must be a number or 'auto', got {adaptive_key!r}")
            return -1
        if isinstance(adaptive_key, bool) or not isinstance(adaptive_key, (int, float, np.integer, np.floating)) or \
                float(adaptive_key) != int(adaptive_key) or not 0 <= int(adaptive_key) <= max_key:
            raise ValueError(f"{what} must be 'auto' or a whole number in 0..{max_key}, got {adaptive_key!r}")
        return int(adaptive_key)

    def enhance_keyed(self, audio, sample_rate, f0, hop_size, adaptive_key="auto", silence_front=0, max_key=12, rand_ini=None,
                      plan=None):
        """S rows, each with an adaptive key of its own, in ONE pass with no host synchronisation: audio (S, T), f0 (S, Fr, 1)
        -> (enhanced (S, T'_max), enhancer sample rate, n_out (S,) int32 device, key (S,) int32 device).  Row s holds
        `enhance(audio[s:s+1], sample_rate, f0[s:s+1], hop_size, adaptive_key=key[s], silence_front=silence_front)` in
        [:n_out[s]] (front cut and front pad included) and exactly 0 after it.
        adaptive_key: 'auto' (the reference's rule per row, on the device: `ddsp_enhancer_keys`), one whole number, or a (S,)
        int32 device tensor of requests (-1 = 'auto').  Keys are clamped to max_key (0..12; the reference has no cap: see
        `KeyedPlan`).  `plan`: the `KeyedPlan` of this geometry (`keyed_plan`); with one, the call uploads nothing and can be
        captured in a HIP graph - then pass `rand_ini` (9,) or (S, 9) as a DEVICE tensor too (None draws on the host)."""
        if audio.dim() != 2 or f0.dim() != 3 or f0.shape[0] != audio.shape[0] or f0.shape[2] != 1:
            raise ValueError("enhance_keyed: audio must be (S, T) and f0 (S, Fr, 1)")
        S, T = audio.shape
        Fr = f0.shape[1]
        if plan is None:
            plan = KeyedPlan(self, T, Fr, sample_rate, hop_size, silence_front, max_key)
        elif (plan.T, plan.Fr, plan.sample_rate, plan.hop_size, plan.silence_front, plan.max_key) != \
                (T, Fr, int(sample_rate), hop_size, silence_front, max_key):
            raise ValueError("enhance_keyed: this KeyedPlan was made for another geometry")
        request = None
        if isinstance(adaptive_key, torch.Tensor):
            if adaptive_key.dtype != torch.int32 or tuple(adaptive_key.shape) != (S,):
                raise ValueError("enhance_keyed: a tensor of key requests must be (S,) int32")
            request = adaptive_key
        else:
            fixed = self.check_key_request(adaptive_key, plan.max_key)
        if not audio.is_cuda or (request is not None and not request.is_cuda):
            raise RuntimeError("the enhancer runs on a HIP device only (no CPU fallback)")
        dev = audio.device
        c = hipddsp.context_for(dev)
        d = plan.on(dev)
        if request is None:
            request = torch.full((S,), fixed, dtype=torch.int32, device=dev)
        f0 = f0.reshape(S, Fr).float()
        key = c.enhancer_keys(f0, plan.cut_frames, plan.max_key, request.contiguous(), d.thresholds)
        # the five lengths of every row: one gather of the plan's table by the key
        n_res, n_f0, n_frames, n_gen, n_out = d.lengths.index_select(0, key.long()).t().contiguous().unbind(0)
        w_res, w_f0, L, w_gen, w_out = plan.widths
        whole = torch.full((S,), plan.T_cut, dtype=torch.int32, device=dev)
        audio_res = c.resample_keyed(d.rs_in, audio[:, plan.cut_samples:], whole, key)                     # (S, w_res)
        f0_res = c.retime_f0(f0[:, plan.cut_frames:], hop_size / sample_rate, None, None, self.enhancer_hop_size / self.enhancer_sample_rate,
                             w_f0, n_src_dev=torch.full((S,), plan.Fr_cut, dtype=torch.int32, device=dev), n_dst_dev=n_f0,
                             keyed=(key, d.div, d.scale))
        stft = self.enhancer.stft()
        with torch.no_grad():
            mel = stft.get_mel(audio_res, n_samples=RaggedCounts([w_res] * S, w_res, n_res), n_frames=RaggedCounts([L] * S, L, n_frames))
            if rand_ini is None:
                rand_ini = torch.rand(S, 9)
            enhanced = self.enhancer.model(mel, f0_res[:, :L], rand_ini=rand_ini, n_frames=RaggedCounts([L] * S, L, n_frames))
        enhanced = c.resample_keyed(d.rs_out, enhanced.reshape(S, -1), n_gen, key)[:, :w_out]
        if plan.front_pad > 0:
            enhanced = F.pad(enhanced, (plan.front_pad, 0))
            n_out = n_out + plan.front_pad
        return enhanced, self.enhancer_sample_rate, n_out, key

    # -- rows of different length in one batch ---------------------------------------------------------------------------
    def batch_lengths(self, n_samples, sample_rate, work_rate):
        """Host integers a row of n_samples goes through in `enhance` at a working rate: (samples at the working rate,
        f0 frames asked of the re-timing, generator frames, generator samples, output samples at the enhancer's rate) -
        the resampler's length formula, `n // hop + 1`, `STFT.frame_count`, `* hop`, the resampler's again."""
        sr_e, hop_e = int(self.enhancer_sample_rate), int(self.enhancer_hop_size)
        n_res = hipddsp.resample_length(int(n_samples), sample_rate, work_rate)
        frames = self.enhancer.stft().frame_count(n_res)
        n_gen = frames * hop_e
        n_out = hipddsp.resample_length(n_gen, work_rate, sr_e)
        return n_res, n_res // hop_e + 1, frames, n_gen, n_out

    def _enhance_rows(self, audio, sample_rate, f0, hop_size, n_samples, n_f0, key, rand_ini):
        """One ragged pass at one working rate: audio (B, T), f0 (B, Fr) -> (enhanced (B, T'), n_out)."""
        c = hipddsp.context_for(audio.device)
        work_rate, pitch_scale, shrink = self._working_rate(key, None)
        sr_e, hop_e = self.enhancer_sample_rate, self.enhancer_hop_size
        lens = [self.batch_lengths(n, sample_rate, work_rate) for n in n_samples]
        if int(sample_rate) != int(work_rate):
            audio = c.resample(audio, sample_rate, work_rate, 128, n_dev=c.ragged_counts(n_samples))
        n_dst = [l[1] for l in lens]
        f0_res = c.retime_f0(f0, hop_size / sample_rate, pitch_scale, pitch_scale, hop_e / sr_e, max(n_dst),
                             n_src_dev=c.ragged_counts(n_f0), n_dst_dev=c.ragged_counts(n_dst))
        enhanced, _ = self.enhancer(audio, f0_res, rand_ini=rand_ini, n_samples=[l[0] for l in lens])
        if shrink != 0 and int(work_rate) != int(sr_e):
            enhanced = c.resample(enhanced, work_rate, sr_e, 128, n_dev=c.ragged_counts([l[3] for l in lens]))
        return enhanced, [l[4] for l in lens]

    def enhance_batch(self, audio, sample_rate, f0, hop_size, n_samples, adaptive_key=0, rand_ini=None, n_f0=None):
        """Rows of different length through the whole enhancer in one padded batch: audio (B, T) with n_samples[b] samples
        per row, f0 (B, Fr, 1) with n_f0[b] frames per row (default int(n_samples[b] // hop_size), at least 1) ->
        (enhanced (B, T'_max), enhancer sample rate, n_out).  Row b holds `enhance(audio[b:b+1, :n_b], sample_rate,
        f0[b:b+1, :n_f0[b]], hop_size, adaptive_key)` in [:n_out[b]] and exactly 0 after it, whatever audio and f0 hold past
        the row's own end; n_out is computed on the host (`batch_lengths`), nothing is read back for it.  There is no
        `silence_front` (a real-time argument).  A numeric adaptive_key is one working rate for the whole batch; 'auto' reads
        back the rows' f0 maxima once, (B,), then runs one ragged pass per distinct key over the rows that share it.
        rand_ini: None, (9,) or (B, 9)."""
        if audio.dim() != 2:
            raise ValueError("enhance_batch: audio must be (B, T)")
        B, T = audio.shape
        n_samples = hipddsp.check_n_samples(n_samples, B, T)
        f0 = f0.reshape(B, -1)
        Fr = f0.shape[1]
        if n_f0 is None:
            n_f0 = [min(Fr, max(1, int(n // hop_size))) for n in n_samples]
        n_f0 = hipddsp.check_n_frames(n_f0, B, Fr)
        if not audio.is_cuda:
            raise RuntimeError("the enhancer runs on a HIP device only (no CPU fallback)")
        if rand_ini is not None:
            rand_ini = rand_ini.float()
            rand_ini = rand_ini.reshape(1, 9).expand(B, 9) if rand_ini.numel() == 9 else rand_ini.reshape(B, 9)
        if not isinstance(adaptive_key, str):
            out, n_out = self._enhance_rows(audio, sample_rate, f0, hop_size, n_samples, n_f0, adaptive_key, rand_ini)
            return out[:, :max(n_out)], self.enhancer_sample_rate, n_out
        if adaptive_key != "auto":
            raise ValueError(f"adaptive_key must be a number or 'auto', got {adaptive_key!r}")
        # the keys decide tensor LENGTHS: the rows' highest f0 over their own frames is the one read-back, (B,)
        own = torch.arange(Fr, device=f0.device)[None, :] < hipddsp.context_for(audio.device).ragged_counts(n_f0)[:, None]
        peaks = torch.where(own, f0.float(), torch.full_like(f0, -float("inf"), dtype=torch.float32)).amax(dim=1).cpu()
        keys = [max(0, float(np.ceil(12 * np.log2(float(p) / 760)))) if float(p) > 0 else 0 for p in peaks]
        print("auto_adaptive_key: " + str([int(k) for k in keys]))
        parts, n_out = {}, [0] * B
        for key in sorted(set(keys)):
            idx = [b for b in range(B) if keys[b] == key]
            sel = torch.tensor(idx, device=audio.device)
            width = max(n_samples[b] for b in idx)
            got, n_rows = self._enhance_rows(audio.index_select(0, sel)[:, :width].contiguous(), sample_rate,
                                             f0.index_select(0, sel), hop_size, [n_samples[b] for b in idx],
                                             [n_f0[b] for b in idx], key, None if rand_ini is None else rand_ini[idx])
            parts[key] = (idx, sel, got)
            for b, n in zip(idx, n_rows):
                n_out[b] = n
        out = torch.zeros(B, max(n_out), device=audio.device, dtype=torch.float32)
        for idx, sel, got in parts.values():
            w = min(got.shape[1], out.shape[1])          # (a group's padded width may exceed every row's own length)
            out[sel, :w] = got[:, :w]
        return out, self.enhancer_sample_rate, n_out
