"""The reference's silence slicer (`slicer.py`) on the device: frame RMS and the tagging state machine are the two kernels of
`ddsp_slicer` (csrc/slicer.hip); this module is the reference's surface around them.

`Slicer` takes the reference's arguments and does its rounding arithmetic; `slice` returns the reference's dict of chunks.
The reference takes its frame RMS from `librosa.feature.rms`, whose centre padding changed from 'reflect' to 'constant' in
librosa 0.10; the reference does not pin a version, so `pad_mode` selects ('constant', the current one, by default).  The
state machine is pinned bit for bit against the reference's own class, the RMS against librosa's documented definition
(tests/golden/make_golden_slicer.py).  Not here: stereo input (the reference's `len(waveform)` on a (2, T) array is the
channel count, a bug) and `chunks2audio` (file I/O).
"""
import numpy as np
import torch

import hipddsp


class Slicer:
    def __init__(self, sr: int, threshold: float = -40., min_length: int = 5000, min_interval: int = 300, hop_size: int = 20,
                 max_sil_kept: int = 5000, pad_mode: str = 'constant', device=None):
        """The reference's arguments (dB, milliseconds) and its two refusals; the frame values are rounded as
        `slicer.py:12-18` rounds them.  `device`: where numpy input is cut (default: the current HIP device; a device tensor is
        cut where it lives)."""
        if not min_length >= min_interval >= hop_size:
            raise ValueError('The following condition must be satisfied: min_length >= min_interval >= hop_size')
        if not max_sil_kept >= hop_size:
            raise ValueError('The following condition must be satisfied: max_sil_kept >= hop_size')
        if pad_mode not in hipddsp.SLICER_PAD:
            raise ValueError(f"pad_mode must be one of {sorted(hipddsp.SLICER_PAD)}, got {pad_mode!r}")
        min_interval = sr * min_interval / 1000
        self.threshold = 10 ** (threshold / 20.)
        self.hop_size = round(sr * hop_size / 1000)
        if self.hop_size < 1:
            raise ValueError(f"hop_size = {hop_size} ms is less than one sample at {sr} Hz")
        self.win_size = min(round(min_interval), 4 * self.hop_size)
        self.min_length = round(sr * min_length / 1000 / self.hop_size)
        self.min_interval = round(min_interval / self.hop_size)
        self.max_sil_kept = round(sr * max_sil_kept / 1000 / self.hop_size)
        if self.win_size < 1 or self.min_interval < 1:
            raise ValueError(f"min_interval = {min_interval / sr * 1000} ms is less than one frame of {self.hop_size} samples")
        self.pad_mode = pad_mode
        self.device = device

    def _device_audio(self, audio):
        if isinstance(audio, np.ndarray):
            audio = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32))
        if not isinstance(audio, torch.Tensor):
            raise ValueError("the slicer takes a numpy array or a tensor")
        dev = audio.device if audio.is_cuda else torch.device(self.device if self.device is not None else "cuda")
        return audio.to(dev, torch.float32)

    def frames(self, n):
        """RMS frames of a row of n samples."""
        return hipddsp.slicer_frames(n, self.win_size, self.hop_size)

    def chunks(self, audio, n_samples=None):
        """audio (T,) or (B, T), numpy or tensor; `n_samples`: the rows' own sample counts (ints on the host, 1 <= n <= T) for
        a ragged batch -> (table (B, capacity, 3) int32 rows start_sample, end_sample, is_silence in the reference's order,
        zero-length chunks included; count (B,) int32; rms (B, frames(T)) fp32), device tensors; nothing is read back.  Row b
        is the row cut alone; table rows from count[b] on and rms values from frames(n_b) on are zeros."""
        x = self._device_audio(audio)
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2 or x.shape[1] < 1:
            raise ValueError(f"the slicer takes audio (T,) or (B, T) with T >= 1, got {tuple(x.shape)}")
        ctx = hipddsp.context_for(x.device)
        n_dev = None
        if n_samples is not None:
            n_dev = ctx.ragged_counts(hipddsp.check_n_samples(n_samples, x.shape[0], x.shape[1], hipddsp.slicer_rule))
        return ctx.slicer(x, self.win_size, self.hop_size, self.threshold, self.min_length, self.min_interval, self.max_sil_kept,
                          pad_mode=self.pad_mode, n_dev=n_dev)

    def chunk_rows(self, waveform):
        """One (T,) waveform -> its chunks as a (K, 3) numpy int32 array (start_sample, end_sample, is_silence): `chunks` and
        ONE read-back of table and count."""
        if getattr(waveform, "ndim", 1) != 1:
            raise ValueError("the slicer takes mono audio of shape (T,); mix the channels down first "
                             f"(got shape {tuple(waveform.shape)})")
        if waveform.shape[0] == 0:
            return np.zeros((1, 3), dtype=np.int32)
        table, count, _ = self.chunks(waveform)
        ctx = hipddsp.context_for(table.device)
        host = torch.cat([count, table.reshape(-1)]).cpu().numpy()
        ctx.poll_error()
        return host[1:].reshape(-1, 3)[:host[0]]

    def slice(self, waveform):
        """The reference's `Slicer.slice`: {"0": {"slice": is_silence, "split_time": "start,end"}, ...}."""
        return {str(k): {"slice": bool(s), "split_time": f"{int(a)},{int(b)}"}
                for k, (a, b, s) in enumerate(self.chunk_rows(waveform))}


def cut(audio, sr, db_thresh=-30, min_len=5000):
    """The reference's `cut` in its `flask_mode` form: the chunks of `audio` (T,) at `sr`."""
    return Slicer(sr=sr, threshold=db_thresh, min_length=min_len).slice(audio)
