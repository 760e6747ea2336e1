"""Shared by tests/golden/make_golden_slicer.py, tests/test_slicer_host.py and tests/test_gpu_slicer.py: the seeded signals of
the silence slicer's cases, and a numpy restatement of the two stages - the frame RMS as librosa documents it
(`librosa.feature.rms(y=, frame_length=, hop_length=)`: centre padding by frame_length // 2, 'constant' since librosa 0.10 and
'reflect' before, framing, sqrt(mean(|x|^2))) in fp32 and in fp64, and the tagging state machine of the reference's
`Slicer.slice` (`slicer.py:32-111`) with its quirks.  The tagger also reports which of its paths a signal took and every
argmin range it evaluated, which is what the condition on the cases (`check_conditions`) is stated on."""
import numpy as np

SR = 8000
# parameter sets in milliseconds, as the constructor takes them; the frame values they round to at 8 kHz (hop 80):
#   base: win 320 (4 hops), min_length 20, min_interval 6, max_sil_kept 10 frames
#   m25:  win 200 (2.5 hops: no multiple of the hop), min_interval round(2.5) = 2
#   odd:  win 201 (odd), min_interval round(2.5125) = 3
#   keep: base with max_sil_kept 30 > min_length: a run from frame 0 can be tagged by the middle rule
#   split: what `main.split(audio, 8000, hop, -40, 300)` constructs - hop 160, win 640, min_length 15, min_interval 15,
#          max_sil_kept 250
PARAMS = {
    "base": dict(sr=SR, threshold=-40.0, min_length=200, min_interval=60, hop_size=10, max_sil_kept=100),
    "m25": dict(sr=SR, threshold=-40.0, min_length=200, min_interval=25, hop_size=10, max_sil_kept=100),
    "odd": dict(sr=SR, threshold=-40.0, min_length=200, min_interval=25.125, hop_size=10, max_sil_kept=100),
    "keep": dict(sr=SR, threshold=-40.0, min_length=200, min_interval=60, hop_size=10, max_sil_kept=300),
    "split": dict(sr=SR, threshold=-40, min_length=300),
}
DEFAULTS = dict(threshold=-40.0, min_length=5000, min_interval=300, hop_size=20, max_sil_kept=5000)   # the reference's
PAD_MODES = ("constant", "reflect")

# name -> (parameter set, plan, extra samples behind the plan, seed, exact zeros for the silences).  A plan is a string of
# segments in frames (hops): s14 = 14 hops of noise floor, t30 = 30 hops of tone.
CASES = {
    # leading silence longer than max_sil_kept, a short run, a run of the middle branch, a long run, a trailing
    # silence
    "all_a": ("base", "s14 t30 s12 t30 s19 t30 s40 t25 s13", 0, 311, False),
    # starts voiced (a leading voiced chunk), a short run, a run that is long enough but follows its tag too closely, ends voiced
    "all_b": ("base", "t26 s9 t3 s9 t30 s27 t24", 37, 12, False),
    # a leading silence shorter than max_sil_kept (no tag), then the three branches in another order, ends voiced
    "all_c": ("base", "s9 t28 s44 t27 s18 t26 s10 t23", 0, 113, False),
    # a leading silence longer than twice max_sil_kept
    "lead_long": ("base", "s30 t25 s9 t5", 0, 124, False),
    # max_sil_kept > min_length: a leading run of the first branch that the middle rule tags
    "keep": ("keep", "s26 t30 s50 t22 s70 t21", 0, 25, False),
    "silent": ("base", "s60", 0, 14, False),
    "zeros": ("base", "s15 t30 s12 t30 s20 t30 s40 t25 s12", 0, 15, True),
    "one_hop": ("base", "t1", 0, 16, False),
    "sub_hop": ("base", "s0", 50, 17, False),
    "early": ("base", "s0", 20, 18, False),
    "ragged_n": ("base", "s13 t30 s14 t29 s9", 61, 19, False),
    "m25_a": ("m25", "s14 t30 s8 t30 s16 t30 s40 t25 s9", 0, 20, False),
    "m25_b": ("m25", "t25 s6 t3 s5 t30 s17 t22", 33, 21, False),
    "odd_a": ("odd", "s14 t30 s8 t30 s16 t30 s40 t25 s9", 0, 22, False),
    "odd_b": ("odd", "t24 s7 t30 s25 t21 s5", 79, 23, False),
    "split_a": ("split", "t20 s22 t25 s3 t20 s20", 0, 26, False),
}
# the paths of the state machine that the cases must take between them (the tagger's `paths`)
ALL_PATHS = ("early", "no_tags", "lead_long", "lead_short", "run_le_keep", "run_le_2keep", "run_longer", "run_not_sliced",
             "trailing", "trailing_short", "lead_voiced_chunk", "closing_chunk", "ends_in_tag", "tag_from_zero")


def frames_of(params):
    """The constructor's rounding arithmetic (`slicer.py:12-18`) -> dict of hop, win (samples), min_length, min_interval,
    max_sil_kept (frames) and the linear threshold."""
    params = {**DEFAULTS, **params}
    sr = params["sr"]
    mi = sr * params["min_interval"] / 1000
    hop = round(sr * params["hop_size"] / 1000)
    return dict(hop=hop, win=min(round(mi), 4 * hop), min_length=round(sr * params["min_length"] / 1000 / hop),
                min_interval=round(mi / hop), max_sil_kept=round(sr * params["max_sil_kept"] / 1000 / hop),
                threshold=10 ** (params["threshold"] / 20.0))


def signal(name):
    """The case's fp32 signal: 220 Hz tone bursts at 0.3 and noise floors near 1e-4 (a seeded level per segment and a seeded
    gain per hop, so that no two frames of a floor are alike), or exact zeros."""
    pset, plan, extra, seed, zeros = CASES[name]
    hop = frames_of(PARAMS[pset])["hop"]
    rng = np.random.Generator(np.random.PCG64(seed))
    parts = []
    for seg in plan.split():
        n = int(seg[1:]) * hop
        if seg[0] == "t":
            parts.append(np.full(n, np.nan))
        else:
            level = 1e-4 * (0.5 + rng.random())
            gain = np.repeat(0.6 + 0.8 * rng.random(n // hop), hop)
            parts.append(np.zeros(n) if zeros else level * gain * rng.standard_normal(n))
    level = 1e-4 * (0.5 + rng.random())
    parts.append(level * rng.standard_normal(extra))
    x = np.concatenate(parts)
    t = np.arange(x.shape[0])
    tone = 0.3 * np.sin(2 * np.pi * 220.0 * t / SR + 0.5)
    return np.where(np.isnan(x), tone, x).astype(np.float32)


def n_frames(n, win, hop):
    return 1 + (n + 2 * (win // 2) - win) // hop


def rms(x, win, hop, pad_mode="constant", dtype=np.float64):
    """librosa.feature.rms(y=x, frame_length=win, hop_length=hop, pad_mode=pad_mode)[0] from its documented definition;
    products, mean and root in `dtype` (np.float32: what librosa gives for fp32 audio; np.float64: the yardstick)."""
    y = np.pad(np.asarray(x, dtype=dtype), win // 2, mode=pad_mode)
    F = 1 + (y.shape[0] - win) // hop
    frames = np.lib.stride_tricks.as_strided(y, shape=(win, F), strides=(y.strides[0], hop * y.strides[0]))
    return np.sqrt(np.mean(np.abs(frames) ** 2, axis=0, dtype=dtype)).astype(dtype)


def tag(r, n, fr):
    """The state machine over the frame RMS `r` of a row of `n` samples, `fr` = frames_of(...) ->
    dict(chunks (K, 3) int64 rows start_sample, end_sample, is_silence; tags; paths: set of names out of ALL_PATHS;
    ranges: [(lo, hi)] every argmin range evaluated, clipped at the array's end as a Python slice is)."""
    hop, thr = fr["hop"], fr["threshold"]
    ML, MI, M = fr["min_length"], fr["min_interval"], fr["max_sil_kept"]
    paths, ranges = set(), []
    if n <= ML:                       # a sample count against a frame count: the reference's comparison
        paths.add("early")
        return dict(chunks=np.array([[0, n, 0]], dtype=np.int64), tags=[], paths=paths, ranges=ranges)
    F = r.shape[0]

    def argmin(lo, hi):
        hi = min(hi, F)
        ranges.append((lo, hi))
        return lo + int(np.argmin(r[lo:hi]))

    tags, start, clip = [], None, 0
    for i in range(F):
        if r[i] < thr:
            if start is None:
                start = i
            continue
        if start is None:
            continue
        leading = start == 0 and i > M
        middle = i - start >= MI and i - clip >= ML
        if not leading and not middle:
            paths.add("lead_short" if start == 0 else "run_not_sliced")
            start = None
            continue
        if leading:
            paths.add("lead_long")
        if start == 0:
            paths.add("tag_from_zero")
        if i - start <= M:
            paths.add("run_le_keep")
            pos = argmin(start, i + 1)
            tags.append((0 if start == 0 else pos, pos))
            clip = pos
        elif i - start <= 2 * M:
            paths.add("run_le_2keep")
            pos = argmin(i - M, start + M + 1)
            pos_l = argmin(start, start + M + 1)
            pos_r = argmin(i - M, i + 1)
            tags.append((0, pos_r) if start == 0 else (min(pos_l, pos), max(pos_r, pos)))
            clip = tags[-1][1]
        else:
            paths.add("run_longer")
            pos_l = argmin(start, start + M + 1)
            pos_r = argmin(i - M, i + 1)
            tags.append((0 if start == 0 else pos_l, pos_r))
            clip = pos_r
        start = None
    if start is not None:
        if F - start >= MI:
            paths.add("trailing")
            tags.append((argmin(start, min(F, start + M) + 1), F + 1))
        else:
            paths.add("trailing_short")
    if not tags:
        paths.add("no_tags")
        return dict(chunks=np.array([[0, n, 0]], dtype=np.int64), tags=tags, paths=paths, ranges=ranges)
    chunks = []
    if tags[0][0]:
        paths.add("lead_voiced_chunk")
        chunks.append((0, min(n, tags[0][0] * hop), 0))
    for k, (a, b) in enumerate(tags):
        if k:
            chunks.append((tags[k - 1][1] * hop, min(n, a * hop), 0))
        chunks.append((a * hop, min(n, b * hop), 1))
    if tags[-1][1] * hop < n:
        paths.add("closing_chunk")
        chunks.append((tags[-1][1] * hop, n, 0))
    else:
        paths.add("ends_in_tag")
    return dict(chunks=np.array(chunks, dtype=np.int64), tags=tags, paths=paths, ranges=ranges)


def restate(name, pad_mode, dtype=np.float64):
    """The case through both stages -> (signal, frame values, rms, the tagger's dict)."""
    fr = frames_of(PARAMS[CASES[name][0]])
    x = signal(name)
    r = rms(x, fr["win"], fr["hop"], pad_mode, dtype)
    return x, fr, r, tag(r, x.shape[0], fr)


def chunk_dict(chunks):
    """(K, 3) chunk rows -> the dict `Slicer.slice` returns."""
    return {str(k): {"slice": bool(s), "split_time": f"{int(a)},{int(b)}"} for k, (a, b, s) in enumerate(chunks)}


def chunks_of_dict(d):
    """The dict `Slicer.slice` returns -> (K, 3) int64 chunk rows."""
    rows = []
    for k in range(len(d)):
        a, b = d[str(k)]["split_time"].split(",")
        rows.append((int(a), int(b), int(bool(d[str(k)]["slice"]))))
    return np.array(rows, dtype=np.int64)


MARGIN = 1e-3
# 4 x the largest relative difference between the fp32 and the fp64 restatement of the frame RMS over all cases and both pad
# modes (measured: 1.07e-7); the GPU test's tolerance on the device RMS against the fp64 restatement
RMS_RTOL = 4.3e-7


def rms_difference(got, want):
    """The largest relative difference of the frame values `got` from the fp64 values `want`; a frame of exact digital
    silence must be exactly 0."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.all(got[want == 0] == 0)
    nz = want > 0
    return float(np.max(np.abs(got[nz] - want[nz]) / want[nz])) if nz.any() else 0.0


def check_conditions(name, pad_mode):
    """The condition under which fp32 summation order cannot change a decision, asserted on the fp64 restatement: every
    frame's RMS is further than 1e-3 (relative) from the threshold, and in every argmin range the state machine evaluates the
    minimum either equals the runner-up exactly (digital silence: the lowest index wins) or lies below it by more than 1e-3."""
    _, fr, r, t = restate(name, pad_mode, np.float64)
    thr = fr["threshold"]
    assert np.all(np.abs(r - thr) > MARGIN * thr), (name, pad_mode, "a frame sits on the threshold")
    for lo, hi in t["ranges"]:
        assert hi > lo, (name, pad_mode, lo, hi)
        v = np.sort(r[lo:hi])
        if v.shape[0] > 1:
            assert v[0] == v[1] or v[0] < v[1] * (1 - MARGIN), (name, pad_mode, lo, hi, v[:2])
    return t


def capacity(F_max, min_interval):
    """The chunk table's rows for a row of at most F_max frames (the bound derived in include/ddsp_amd.h): at most
    F_max // min_interval tags that each need their own silent run of min_interval frames, one more by the leading rule, and
    2 K + 1 chunks for K tags."""
    return 2 * (F_max // max(1, min_interval) + 1) + 1
