"""Weights, audio and a CPU restatement of the CREPE f0 extractor (ddsp/crepe.py, ddsp.vocoder.F0_Extractor), shared by the
CREPE tests and tests/golden/make_golden_crepe.py.

The weight fill is deterministic and independent of torch's generator: per state-dict key, numpy's default generator seeded
with the CRC-32 of the key draws N(0, 1) values, scaled as
  batch-norm gains (`..._BN.weight`)      1 + 0.1 N
  running variances                       0.5 + |N| (positive)
  biases, shifts and running means        0.05 N
  every other weight                      N / sqrt(fan_in), fan_in = the numel of one output row
  `num_batches_tracked`                   0

The restatement (fp64 network in PyTorch functional ops, numpy Viterbi over the full 360 x 360 transition matrix, numpy
post-filter) follows the published algorithms: torchcrepe's preprocess / infer / postprocess with the Viterbi decoder
(librosa.sequence.viterbi) and the reference's median / threshold / masked-average filter."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

BINS = 360
HOP = 80
WIN = 1024
CENTS_OFFSET = 1997.3794084376191
BN_EPS = 0.0010000000474974513
TINY = np.float32(np.finfo(np.float32).tiny)
WIDTHS = {"full": (1024, 128, 128, 128, 256, 512), "tiny": (128, 16, 16, 16, 32, 64)}
KERNELS = (512, 64, 64, 64, 64, 64)

# name -> (B, T at 16 kHz, seed, kind): a voiced sweep plus noise, silence, a length that is not a multiple of 80, a batch of 2
CASES = {"sweep": (1, 8000, 21, "sweep"), "silence": (1, 4000, 22, "silence"), "odd": (1, 6397, 23, "sweep"),
         "pair": (2, 4800, 24, "sweep")}


def state_dict_shapes(model="full"):
    """torchcrepe's `Crepe(model)` state-dict keys (registration order) -> shapes."""
    w = WIDTHS[model]
    c_in = (1,) + w[:-1]
    out = {}
    for i in range(6):
        out[f"conv{i + 1}.weight"] = (w[i], c_in[i], KERNELS[i], 1)
        out[f"conv{i + 1}.bias"] = (w[i],)
        for k in ("weight", "bias", "running_mean", "running_var"):
            out[f"conv{i + 1}_BN.{k}"] = (w[i],)
        out[f"conv{i + 1}_BN.num_batches_tracked"] = ()
    out["classifier.weight"] = (BINS, 4 * w[5])
    out["classifier.bias"] = (BINS,)
    return out


def fill_one(key, shape):
    if key.endswith("num_batches_tracked"):
        return np.array(0, dtype=np.int64)
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    n = rng.standard_normal(shape)
    if key.endswith("_BN.weight"):
        a = 1.0 + 0.1 * n
    elif key.endswith("running_var"):
        a = 0.5 + np.abs(n)
    elif len(shape) == 1:
        a = 0.05 * n
    else:
        a = n / np.sqrt(int(np.prod(shape[1:])))
    return a.astype(np.float32)


def fill(model="full"):
    """{key: tensor} of the deterministic fill for torchcrepe's 'full' or 'tiny' keys."""
    return {k: torch.from_numpy(fill_one(k, s)) for k, s in state_dict_shapes(model).items()}


def audio(name):
    """(B, T) float32 16 kHz audio of a case."""
    B, T, seed, kind = CASES[name]
    rng = np.random.default_rng(seed)
    if kind == "silence":
        return torch.zeros(B, T)
    t = np.arange(T) / 16000.0
    rows = []
    for b in range(B):
        f = 110.0 * (1 + b) * np.exp(np.log(4.0) * t / t[-1])          # a two-octave sweep
        ph = 2 * np.pi * np.cumsum(f) / 16000.0
        rows.append(0.3 * np.sin(ph) + 0.15 * np.sin(2 * ph + 0.3) + 0.02 * rng.standard_normal(T))
    return torch.from_numpy(np.stack(rows).astype(np.float32))


# ---- network (fp64, PyTorch functional ops) ---------------------------------------------------------------------
def frames(audio16, hop=HOP):
    """(B, T) -> (B * Fr, 1024) frames of the zero-padded audio (512 each side), Fr = 1 + T // hop, each minus its mean and
    divided by max(1e-10, unbiased std).  Computed in the input's dtype."""
    B, T = audio16.shape
    fr = 1 + T // hop
    x = F.pad(audio16, (WIN // 2, WIN // 2))
    idx = torch.arange(fr)[:, None] * hop + torch.arange(WIN)[None, :]
    fx = x[:, idx].reshape(B * fr, WIN)
    fx = fx - fx.mean(dim=1, keepdim=True)
    return fx / torch.clamp(fx.std(dim=1, keepdim=True), min=1e-10)


def network(sd, fx):
    """frames (N, 1024) -> sigmoid activations (N, 360): six [pad, conv, ReLU, batch norm (eval), 2x1 max-pool] layers and the
    classifier over the (position, channel) features."""
    x = fx[:, None, :, None]
    for i in range(6):
        p = f"conv{i + 1}"
        x = F.pad(x, (0, 0, 254, 254) if i == 0 else (0, 0, 31, 32))
        x = F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], stride=(4, 1) if i == 0 else (1, 1))
        x = F.relu(x)
        x = F.batch_norm(x, sd[p + "_BN.running_mean"], sd[p + "_BN.running_var"], sd[p + "_BN.weight"], sd[p + "_BN.bias"],
                         False, 0.0, BN_EPS)
        x = F.max_pool2d(x, (2, 1), (2, 1))
    x = x.permute(0, 2, 1, 3).reshape(x.shape[0], -1)
    return torch.sigmoid(F.linear(x, sd["classifier.weight"], sd["classifier.bias"]))


def activations64(sd, audio16, hop=HOP):
    """(B, T) -> (B, Fr, 360) in fp64."""
    sd64 = {k: v.double() for k, v in sd.items() if v.dtype.is_floating_point}
    B = audio16.shape[0]
    with torch.no_grad():
        return network(sd64, frames(audio16.double(), hop)).reshape(B, -1, BINS)


# ---- decode ---------------------------------------------------------------------------------------------------
def frequency_to_bin(f, ceil=False):
    """fp32 (1200 log2(f / 10) - 1997.3794084376191) / 20, floored or ceiled (torch.tensor(f) arithmetic)."""
    x = (np.float32(1200) * np.log2(np.float32(f) / np.float32(10)) - np.float32(CENTS_OFFSET)) / np.float32(20)
    return int(np.ceil(x) if ceil else np.floor(x))


def mask_range(fmin, fmax):
    """[lo, hi): the bins left unmasked by probabilities[:, :minidx] = probabilities[:, maxidx:] = -inf (Python slices)."""
    lo = slice(None, frequency_to_bin(fmin)).indices(BINS)[1]
    hi = slice(frequency_to_bin(fmax, ceil=True), None).indices(BINS)[0]
    return lo, hi


def emissions(probs, fmin, fmax):
    """probs (Fr, 360) -> fp32 log(softmax(masked) + tiny) (Fr, 360)."""
    p = np.asarray(probs, dtype=np.float32).copy()
    lo, hi = mask_range(fmin, fmax)
    p[:, :lo] = -np.inf
    p[:, hi:] = -np.inf
    e = np.exp(p - p.max(axis=1, keepdims=True))
    s = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    return np.log(s + TINY).astype(np.float32)


def log_transitions():
    """(360, 360) fp64 log(T + tiny), T[i, j] = max(12 - |i - j|, 0) / row sum."""
    i = np.arange(BINS)
    t = np.maximum(12 - np.abs(i[:, None] - i[None, :]), 0).astype(np.float64)
    t = t / t.sum(axis=1, keepdims=True)
    return np.log(t + np.float64(TINY))


def viterbi_naive(logp):
    """Full-matrix fp64 Viterbi over emissions (Fr, 360) from a uniform start, first index on ties.
    -> (bins (Fr,), margins (Fr,)): margins[t] = the gap between the best and second-best predecessor of the path's state
    at t (t >= 1), margins[0] = the gap of the final argmax."""
    lt = log_transitions()
    n = logp.shape[0]
    v = logp[0].astype(np.float64) + np.log(1.0 / BINS + np.float64(TINY))
    ptr = np.zeros((n, BINS), dtype=np.int64)
    gap = np.zeros((n, BINS))
    for t in range(1, n):
        cand = v[:, None] + lt                      # (from i, to j)
        ptr[t] = np.argmax(cand, axis=0)
        srt = np.sort(cand, axis=0)
        gap[t] = srt[-1] - srt[-2]
        v = logp[t].astype(np.float64) + cand[ptr[t], np.arange(BINS)]
    bins = np.zeros(n, dtype=np.int64)
    bins[-1] = int(np.argmax(v))
    srt = np.sort(v)
    margins = np.zeros(n)
    margins[0] = srt[-1] - srt[-2]
    for t in range(n - 1, 0, -1):
        margins[t] = gap[t, bins[t]]
        bins[t - 1] = ptr[t, bins[t]]
    return bins, margins


def viterbi_banded(logp):
    """The same decode from the 23 in-band candidates plus the out-of-band term value[g] + log(tiny), g = the first global
    argmax of the previous values (the device kernel's form)."""
    lt = log_transitions()
    log_eps = np.log(np.float64(TINY))
    n = logp.shape[0]
    v = logp[0].astype(np.float64) + np.log(1.0 / BINS + np.float64(TINY))
    ptr = np.zeros((n, BINS), dtype=np.int64)
    for t in range(1, n):
        g = int(np.argmax(v))
        nv = np.empty(BINS)
        for j in range(BINS):
            lo, hi = max(0, j - 11), min(BINS, j + 12)
            c = v[lo:hi] + lt[lo:hi, j]
            k = int(np.argmax(c))
            best, bi = c[k], lo + k
            if abs(g - j) > 11:
                o = v[g] + log_eps
                if o > best or (o == best and g < bi):
                    best, bi = o, g
            ptr[t, j] = bi
            nv[j] = np.float64(logp[t, j]) + best
        v = nv
    bins = np.zeros(n, dtype=np.int64)
    bins[-1] = int(np.argmax(v))
    for t in range(n - 1, 0, -1):
        bins[t - 1] = ptr[t, bins[t]]
    return bins


def decode(probs, fmin, fmax, segment=512):
    """probs (Fr, 360) -> (bins, margins) decoded in independent pieces of `segment` frames."""
    e = emissions(probs, fmin, fmax)
    out_b, out_m = [], []
    for s in range(0, e.shape[0], segment):
        b, m = viterbi_naive(e[s:s + segment])
        out_b.append(b)
        out_m.append(m)
    return np.concatenate(out_b), np.concatenate(out_m)


def bin_to_hz(bins):
    """fp32 10 * 2^((20 bin + 1997.3794084376191) / 1200) (no dither)."""
    c = (np.float32(20) * np.asarray(bins).astype(np.float32) + np.float32(CENTS_OFFSET)).astype(np.float32)
    return (np.float32(10) * np.power(np.float32(2), c / np.float32(1200))).astype(np.float32)


def known_path():
    """A bin path the decode must return from bump_track(path) (fmin 50, fmax 1100): plateaus, steps of 8 and 10 bins per frame
    and a glide of half a bin per frame.  An emission favours its bump by at most ~1 nat (a softmax of values in (0, 1)), so an
    out-of-band jump (~87 nats) never pays inside 360 bins: sliding costs ~0.25 nats per bin.  The out-of-band term shows in
    the back-pointers of states far from the best one instead (out_of_band_choices)."""
    return np.concatenate([np.full(60, 100), 100 + 8 * np.arange(1, 11), np.full(60, 180), np.round(180 - 0.5 * np.arange(1, 81)),
                           np.full(40, 140), 140 - 10 * np.arange(1, 7), np.full(60, 80)]).astype(np.int64)


def out_of_band_choices(logp):
    """Number of (t, j) whose best predecessor in the full-matrix decode lies more than 11 bins away."""
    lt = log_transitions()
    v = logp[0].astype(np.float64) + np.log(1.0 / BINS + np.float64(TINY))
    n = 0
    for t in range(1, logp.shape[0]):
        cand = v[:, None] + lt
        p = np.argmax(cand, axis=0)
        n += int((np.abs(p - np.arange(BINS)) > 11).sum())
        v = logp[t].astype(np.float64) + cand[p, np.arange(BINS)]
    return n


def bump_track(n, path, width=1.0):
    """Known-answer activations (n, 360): a Gaussian bump of height 0.95 on bin path[t] over a 0.02 floor."""
    i = np.arange(BINS)[None, :]
    return (0.02 + 0.93 * np.exp(-0.5 * ((i - np.asarray(path)[:, None]) / width) ** 2)).astype(np.float32)


# ---- the reference's post-filter (ddsp/vocoder.py:96-113), restated -----------------------------------------------
def _reflect(i, n):
    return -i if i < 0 else (2 * (n - 1) - i if i >= n else i)


def postfilter(f0, pd, sr, hop, n_frames, start_frame, uv_interp, f0_min, threshold=0.05):
    """f0, pd (Fr,) fp32 -> (n_frames,) fp32: lower median of pd over reflect(i-1..i+2), f0 = NaN where that < threshold, NaN-
    masked mean over reflect(i-1..i+2) (0 when the window has no value), re-timing f0[min(rint(n hop / sr / 0.005), Fr - 1)],
    start_frame zeros in front, then with uv_interp numpy.interp over the zero frames and the clamp to f0_min."""
    f0 = np.asarray(f0, dtype=np.float32)
    pd = np.asarray(pd, dtype=np.float32)
    fr = f0.shape[0]
    if fr < 3:
        raise ValueError("the reflect padding needs at least 3 frames")
    med = np.empty(fr, dtype=np.float32)
    for i in range(fr):
        med[i] = np.sort([pd[_reflect(i + k, fr)] for k in (-1, 0, 1, 2)])[1]
    g = np.where(med < np.float32(threshold), np.float32(np.nan), f0)
    pooled = np.empty(fr, dtype=np.float32)
    for i in range(fr):
        s, c = np.float32(0), np.float32(0)
        for k in (-1, 0, 1, 2):
            v = g[_reflect(i + k, fr)]
            if not np.isnan(v):
                s = np.float32(s + v)
                c = np.float32(c + 1)
        pooled[i] = s / max(c, np.float32(1))
    out = np.zeros(n_frames, dtype=np.float32)
    for n in range(n_frames - start_frame):
        out[start_frame + n] = pooled[min(int(np.rint(n * hop / sr / 0.005)), fr - 1)]
    if uv_interp:
        voiced = np.nonzero(out != 0)[0]
        if len(voiced):
            z = np.nonzero(out == 0)[0]
            out[z] = np.interp(z.astype(np.float64), voiced.astype(np.float64), out[voiced].astype(np.float64))
        out[out < f0_min] = f0_min
    return out


def extract_bookkeeping(T, sr, hop, silence_front):
    """(n_frames, start_frame, first kept sample) of F0_Extractor.extract for T input samples."""
    n_frames = int(T // hop) + 1
    start_frame = int(silence_front * sr / hop)
    return n_frames, start_frame, int(np.round(start_frame * hop / sr * sr))
