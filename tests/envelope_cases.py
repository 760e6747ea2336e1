"""The envelope mix (`ddsp_envelope_rms`, `ddsp_envelope_apply`) stated in numpy fp64, and the cases of its kernel test.
include/ddsp_amd.h states the same rule at the symbols; this file is the kernels' yardstick.

THE RULE is RVC's `change_rms(data1, sr1, data2, sr2, rate)`: data1 the source, data2 the converted output, rate the share of
the output's own envelope that is kept.
  1. Frame RMS as librosa.feature.rms documents it with center=True: a row of n samples has N = 1 + n // hop frames, frame i
     covers [i * hop - win / 2, i * hop + win / 2), samples outside [0, n) count as 0, rms[i] = sqrt(sum x^2 / win),
     win = m * hop, m even in 2..8.
  2. Both envelopes go to the output's length n2 as F.interpolate(mode="linear", align_corners=False) does:
     x = max((t + 0.5) * N / n2 - 0.5, 0), i0 = min(floor(x), N - 1), i1 = min(i0 + 1, N - 1), lam = x - i0,
     e = (1 - lam) * env[i0] + lam * env[i1].
  3. e2 = max(e2, 1e-6); g = e1 ** (1 - rate) * e2 ** (rate - 1); out[t] = data2[t] * g.
A row with rate == 1 or without an owner keeps its bits.  e1 == 0 with rate < 1: the gain is exactly 0."""
import numpy as np

FLOOR = 1e-6
RMS_SETTINGS = ((4, 2), (5, 4))                     # (hop, m)
OFFLINE = (22050, 2, 3 * 22050 + 17)                # (hop, m, n): one workgroup strides a hop-block
LIVE = (441, 4, 8820)                               # a wave strides a hop-block
ENV_GATE = 1e-10                                    # relative, on the envelopes and on the output (plus 1e-300 absolute there)


def rms_lengths(hop):
    return (1, hop - 1, hop, hop + 1, 2 * hop + 3, 37)


def frame_rms(x, hop, m):
    """x (n,) -> rms (1 + n // hop,) fp64: every frame's samples are summed where they lie inside the row."""
    x = np.asarray(x, dtype=np.float64)
    n, win = x.shape[0], m * hop
    N = 1 + n // hop
    out = np.zeros(N, dtype=np.float64)
    for i in range(N):
        lo, hi = max(i * hop - win // 2, 0), min(i * hop + win // 2, n)
        out[i] = np.sqrt(np.sum(x[lo:hi] ** 2) / win)
    return out


def interpolate(env, n2):
    """env (N,) -> (n2,): step 2 of the rule."""
    env = np.asarray(env, dtype=np.float64)
    N = env.shape[0]
    t = np.arange(n2, dtype=np.float64)
    x = np.maximum((t + 0.5) * N / n2 - 0.5, 0.0)
    i0 = np.minimum(np.floor(x).astype(np.int64), N - 1)
    i1 = np.minimum(i0 + 1, N - 1)
    lam = x - i0
    return (1.0 - lam) * env[i0] + lam * env[i1]


def gain(src, hop1, out, hop2, m, rate):
    """The gain of every output sample, (n2,) fp64: steps 1 to 3 for one (source row, output row) and a rate in [0, 1)."""
    n2 = len(out)
    e1 = interpolate(frame_rms(src, hop1, m), n2)
    e2 = np.maximum(interpolate(frame_rms(out, hop2, m), n2), FLOOR)
    return np.power(e1, 1.0 - rate) * np.power(e2, rate - 1.0)


def bad_rate(rate):
    return not (np.isfinite(rate) and 0 <= rate <= 1)


def mix(src, hop1, out, hop2, m, rate):
    """-> the output row after the mix, in its own dtype; its own bits for rate == 1 or a refused rate."""
    out = np.asarray(out)
    if bad_rate(rate) or rate == 1:
        return out.copy()
    return (out.astype(np.float64) * gain(src, hop1, out, hop2, m, rate)).astype(out.dtype)


def signal(n, seed, scale=0.3, dtype=np.float32):
    """A deterministic row with an envelope that moves: noise under a slow swell."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = scale * rng.standard_normal(n) * (0.25 + np.abs(np.sin(t * (3.0 / max(n, 1)) + seed)))
    return x.astype(dtype)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def rel_err(got, want):
    """Largest |got - want| / |want| over the elements with want != 0; elements with want == 0 must be equal."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    zero = want == 0
    if not np.array_equal(got[zero], want[zero]):
        return np.inf
    if zero.all():
        return 0.0
    return float(np.max(np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero])))
