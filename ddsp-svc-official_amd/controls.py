"""The controls of a conversion and the record of an offline job: what a job, or a slot of a `realtime.StreamBank`, may carry
beside its model, speaker and key.  `SpeakerTimeline` (a voice that glides), `KeyTimeline` (a key that moves), `FormantTimeline`
(a formant shift that moves), `PitchTune` (pitch correction), `UnitIndex` / `UnitIndexBank` (unit retrieval) and `EnvelopeMix`
(the source's loudness envelope), each with the builder of the host tables its kernel takes (`timeline_tables`, `key_tables`,
`formant_tables`, `tune_tables`, `index_tables`, `envelope_tables`).  `Job` names the fields of an offline job, and `Job.of` is
the one place that knows the positional (tuple) form.  Host code over `hipddsp`: this module imports neither `infer_offline`
nor `realtime`, which both import it (`infer_offline` re-exports every name, so `infer_offline.X` in a message still names it).
"""
import dataclasses
import math
import numbers
import os

import numpy as np
import torch

import hipddsp


class SpeakerTimeline:
    """The speaker of a job as a function of FILE time: a voice that glides inside a file.  points: a non-empty list of
    (seconds, id | {id: weight}), times non-negative and ascending; between two points the weights of every id are interpolated
    linearly, before the first and after the last they stay (an id a point does not name has weight 0 there; weights are not
    normalised, as the reference's `spk_mix_dict` values are not).  `ids`: the distinct ids in order of first appearance, at most
    `hipddsp.MAX_MIX` - the slots of the per-frame mix.  ValueError for anything else."""

    def __init__(self, points):
        if not (isinstance(points, (list, tuple)) and len(points)):
            raise ValueError("SpeakerTimeline: points must be a non-empty list of (seconds, id | {id: weight})")
        self.points, self.ids, last = [], [], 0.0
        for n, point in enumerate(points):
            if not (isinstance(point, (tuple, list)) and len(point) == 2):
                raise ValueError(f"SpeakerTimeline: point {n} must be (seconds, id | {{id: weight}}), got {point!r}")
            t, spk = point
            if not (isinstance(t, numbers.Real) and not isinstance(t, bool) and t >= 0 and t == t and t != float("inf")):
                raise ValueError(f"SpeakerTimeline: point {n}: the time must be a finite number of seconds >= 0, got {t!r}")
            if t < last:
                raise ValueError(f"SpeakerTimeline: point {n}: times must ascend, {t!r} follows {last!r}")
            last = t
            mix = spk if isinstance(spk, dict) else {spk: 1.0}
            if not mix or not all(isinstance(i, numbers.Integral) and not isinstance(i, bool) and i >= 1 and
                                  isinstance(w, numbers.Real) for i, w in mix.items()):
                raise ValueError(f"SpeakerTimeline: point {n}: a speaker is an id >= 1 or a non-empty {{id: weight}}, got {spk!r}")
            self.points.append((float(t), {int(i): float(w) for i, w in mix.items()}))
            self.ids.extend(int(i) for i in mix if int(i) not in self.ids)
        if len(self.ids) > hipddsp.MAX_MIX:
            raise ValueError(f"SpeakerTimeline: at most {hipddsp.MAX_MIX} distinct ids, got {len(self.ids)}")

    def frames(self, sampling_rate, block_size):
        """-> (breakpoint frames, weights [point][slot of `ids`]): a point's frame is int(round(t * sampling_rate /
        block_size)); ValueError when two points land on one frame (a jump has no slope: move one of them by a frame)."""
        at = [int(round(t * sampling_rate / block_size)) for t, _ in self.points]
        for n in range(1, len(at)):
            if at[n] <= at[n - 1]:
                raise ValueError(f"SpeakerTimeline: points {n - 1} and {n} ({self.points[n - 1][0]} s, {self.points[n][0]} s) both "
                                 f"land on frame {at[n]} at {sampling_rate} Hz and block size {block_size}")
        return at, [[mix.get(i, 0.0) for i in self.ids] for _, mix in self.points]


def timeline_tables(speakers, mine, sampling_rate, block_size):
    """The tables `ddsp_mix_timeline` takes for the jobs `mine` (indices into `speakers`, one model's jobs) -> CPU tensors
    (bp_off (J + 1,) int32, bp_frame (P,) int32, bp_w (P, K) fp32, job_ids (J, K) int32) over ALL J jobs - a row names its job
    by its number in the call -, K the most slots of a job among `mine`.  A `SpeakerTimeline` gives its breakpoints; an id or a
    mix dict is the one breakpoint at frame 0 (a constant mix); a job outside `mine` owns no breakpoint.  Short rows are padded
    with {id 1, weight 0}."""
    per_job = {}
    for j in mine:
        s = speakers[j]
        if isinstance(s, SpeakerTimeline):
            at, w = s.frames(sampling_rate, block_size)
            per_job[j] = (list(s.ids), at, w)
        else:
            mix = s if isinstance(s, dict) else {s: 1.0}
            per_job[j] = ([int(i) for i in mix], [0], [[float(v) for v in mix.values()]])
    K = max(len(ids) for ids, _, _ in per_job.values())
    off, frame, w, job_ids = [0], [], [], []
    for j in range(len(speakers)):
        ids, at, rows = per_job.get(j, ([], [], []))
        frame.extend(at)
        w.extend(row + [0.0] * (K - len(row)) for row in rows)
        job_ids.append(ids + [1] * (K - len(ids)))
        off.append(len(frame))
    return (torch.tensor(off, dtype=torch.int32), torch.tensor(frame, dtype=torch.int32),
            torch.tensor(w, dtype=torch.float32).reshape(-1, K), torch.tensor(job_ids, dtype=torch.int32).reshape(-1, K))


class KeyTimeline:
    """The key of a job as a function of FILE time (of a bank's slot: of stream time, `StreamBank.set_pitch_timeline`): a key
    that moves.  points: a non-empty list of (seconds, semitones), times finite, non-negative and ascending, semitones finite.
    The key is linear IN SEMITONES between two points and stays before the first and after the last; the f0 factor is
    2 ** (key / 12).  A timeline of one point is a constant key, with that key's bits (include/ddsp_amd.h states the rule at
    `ddsp_pieces_gather_keys`).  ValueError for anything else."""

    def __init__(self, points):
        if not (isinstance(points, (list, tuple)) and len(points)):
            raise ValueError("KeyTimeline: points must be a non-empty list of (seconds, semitones)")
        self.points, last = [], 0.0
        for n, point in enumerate(points):
            if not (isinstance(point, (tuple, list)) and len(point) == 2):
                raise ValueError(f"KeyTimeline: point {n} must be (seconds, semitones), got {point!r}")
            t, key = point
            if not (isinstance(t, numbers.Real) and not isinstance(t, bool) and t >= 0 and t == t and t != float("inf")):
                raise ValueError(f"KeyTimeline: point {n}: the time must be a finite number of seconds >= 0, got {t!r}")
            if t < last:
                raise ValueError(f"KeyTimeline: point {n}: times must ascend, {t!r} follows {last!r}")
            last = t
            if not (isinstance(key, numbers.Real) and not isinstance(key, bool) and key == key and abs(key) != float("inf")):
                raise ValueError(f"KeyTimeline: point {n}: the key must be a finite number of semitones, got {key!r}")
            self.points.append((float(t), float(key)))

    def frames(self, sampling_rate, block_size):
        """-> (breakpoint frames, semitones): `SpeakerTimeline.frames`' rule - a point's frame is int(round(t * sampling_rate /
        block_size)); ValueError when two points land on one frame (a jump has no slope: move one of them by a frame)."""
        at = [int(round(t * sampling_rate / block_size)) for t, _ in self.points]
        for n in range(1, len(at)):
            if at[n] <= at[n - 1]:
                raise ValueError(f"KeyTimeline: points {n - 1} and {n} ({self.points[n - 1][0]} s, {self.points[n][0]} s) both "
                                 f"land on frame {at[n]} at {sampling_rate} Hz and block size {block_size}")
        return at, [key for _, key in self.points]


def key_tables(keys, sampling_rate, block_size):
    """The tables `ddsp_pieces_gather_keys` takes for the J jobs whose keys are `keys` (a number of semitones or a `KeyTimeline`
    each) -> CPU tensors (bp_off (J + 1,) int32, bp_frame (P,) int32, bp_semi (P,) fp32, bp_fac (P,) fp32).  A `KeyTimeline`
    gives its breakpoints in file frames; a number is the one breakpoint at frame 0.  Every breakpoint's factor is
    2 ** (float(key) / 12), a Python float stored to fp32: `job_table`'s `key_factor` of a constant key."""
    off, frame, semi = [0], [], []
    for key in keys:
        at, values = key.frames(sampling_rate, block_size) if isinstance(key, KeyTimeline) else ([0], [float(key)])
        frame.extend(at)
        semi.extend(values)
        off.append(len(frame))
    return (torch.tensor(off, dtype=torch.int32), torch.tensor(frame, dtype=torch.int32), torch.tensor(semi, dtype=torch.float32),
            torch.tensor([2 ** (float(k) / 12) for k in semi], dtype=torch.float32))


MAX_FORMANT = 24.0   # semitones, either way (`ddsp.vocoder` holds a numeric shift to the same bound)


class FormantTimeline(KeyTimeline):
    """The formant shift of a job as a function of FILE time: points (seconds, semitones) under `KeyTimeline`'s validation and
    frame rule, |semitones| <= 24.  The shift is linear in semitones between two points and held outside them; the factor of a
    frame is the key timeline rule's (include/ddsp_amd.h at `ddsp_pieces_gather_keys`) - what that kernel multiplies onto an f0
    of 1.0 at that file frame.  It is a job's fifth entry, never its key.  ValueError for anything else."""

    def __init__(self, points):
        try:
            super().__init__(points)
        except ValueError as e:
            raise ValueError(str(e).replace("KeyTimeline", "FormantTimeline").replace("the key must", "the shift must")) from None
        for n, (_, semi) in enumerate(self.points):
            if abs(semi) > MAX_FORMANT:
                raise ValueError(f"FormantTimeline: point {n}: the shift must lie within +-{MAX_FORMANT:g} semitones, got {semi!r}")

    def frames(self, sampling_rate, block_size):
        try:
            return super().frames(sampling_rate, block_size)
        except ValueError as e:
            raise ValueError(str(e).replace("KeyTimeline", "FormantTimeline")) from None


def formant_tables(formants, sampling_rate, block_size):
    """`key_tables` for `job_formants`' list: a job without a shift is the one breakpoint of 0 semitones, factor 1."""
    return key_tables([0.0 if f is None else f for f in formants], sampling_rate, block_size)


NOTE_NAMES = {"C": 0, "D": 2, "E": 4, "F": 5, "G": 7, "A": 9, "B": 11}
SCALES = {"major": (0, 2, 4, 5, 7, 9, 11), "minor": (0, 2, 3, 5, 7, 8, 10), "chromatic": tuple(range(12)),
          "major_pentatonic": (0, 2, 4, 7, 9), "minor_pentatonic": (0, 3, 5, 7, 10)}


def pitch_class(note):
    """A pitch class 0..11 (C = 0) as it is, or a note name - a letter A-G, then any number of '#' or 'b' - as its class.
    ValueError for anything else."""
    if isinstance(note, numbers.Integral) and not isinstance(note, bool) and 0 <= note <= 11:
        return int(note)
    if isinstance(note, str) and note and note[0].upper() in NOTE_NAMES and set(note[1:]) <= {"#", "b"}:
        return (NOTE_NAMES[note[0].upper()] + note.count("#") - note[1:].count("b")) % 12
    raise ValueError(f"a note is a pitch class 0..11 or a name such as 'A', 'F#' or 'Bb', got {note!r}")


class PitchTune:
    """Pitch correction of a job (its sixth entry) or of a bank's slot (`StreamBank.set_tune`): the sung f0 is pulled toward the
    nearest allowed note (include/ddsp_amd.h states the rule at `ddsp_f0_tune`).  notes: an iterable of pitch classes 0..11
    (C = 0) or note names, at least one; strength in [0, 1]: the share of the correction that is applied; retune: seconds, the
    time constant at which the correction follows a new note (0: at once - with strength 1 that is hard tuning); a4: the Hz of
    A4.  ValueError for an empty note set, a strength outside [0, 1], a negative or non-finite retune, or an a4 that is not a
    finite number > 0."""

    def __init__(self, notes, strength=1.0, retune=0.05, a4=440.0):
        if isinstance(notes, (str, numbers.Number)):
            raise ValueError(f"PitchTune: notes must be an iterable of pitch classes or note names, got {notes!r}")
        try:
            classes = sorted({pitch_class(n) for n in notes})
        except TypeError:
            raise ValueError(f"PitchTune: notes must be an iterable of pitch classes or note names, got {notes!r}") from None
        except ValueError as e:
            raise ValueError(f"PitchTune: {e}") from None
        if not classes:
            raise ValueError("PitchTune: the note set is empty")

        def real(x):
            return isinstance(x, numbers.Real) and not isinstance(x, bool) and math.isfinite(x)
        if not (real(strength) and 0 <= strength <= 1):
            raise ValueError(f"PitchTune: strength must be a number in [0, 1], got {strength!r}")
        if not (real(retune) and retune >= 0):
            raise ValueError(f"PitchTune: retune must be a finite number of seconds >= 0, got {retune!r}")
        if not (real(a4) and a4 > 0):
            raise ValueError(f"PitchTune: a4 must be a finite number of Hz > 0, got {a4!r}")
        self.notes, self.strength, self.retune, self.a4 = tuple(classes), float(strength), float(retune), float(a4)
        self.mask = sum(1 << p for p in classes)

    @classmethod
    def scale(cls, tonic, kind="major", **kw):
        """The scale of `kind` - major, minor (natural), chromatic, major_pentatonic, minor_pentatonic - on `tonic` (a pitch
        class or a note name); the keywords are the constructor's."""
        if kind not in SCALES:
            raise ValueError(f"PitchTune.scale: kind must be one of {', '.join(SCALES)}, got {kind!r}")
        try:
            root = pitch_class(tonic)
        except ValueError as e:
            raise ValueError(f"PitchTune.scale: {e}") from None
        return cls([(root + step) % 12 for step in SCALES[kind]], **kw)

    @classmethod
    def named(cls, text, **kw):
        """'A minor', 'F# major_pentatonic', 'C' (major): `scale` from one string, as main.py's options take it."""
        words = text.split() if isinstance(text, str) else []
        if not 1 <= len(words) <= 2:
            raise ValueError(f"PitchTune.named: a scale is '<tonic> [<kind>]' such as 'A minor', got {text!r}")
        return cls.scale(words[0], *words[1:], **kw)

    def setting(self, hop_seconds):
        """-> (mask, (a4, strength, alpha)) as `ddsp_f0_tune` takes them for frames `hop_seconds` apart:
        alpha = 1 - exp(-hop_seconds / retune), 1 for a retune of 0 (and where the quotient is so large that exp gives 0)."""
        if not (isinstance(hop_seconds, numbers.Real) and math.isfinite(hop_seconds) and hop_seconds > 0):
            raise ValueError(f"PitchTune.setting: hop_seconds must be a finite number > 0, got {hop_seconds!r}")
        alpha = 1.0 if self.retune == 0 else -math.expm1(-float(hop_seconds) / self.retune)
        return self.mask, (self.a4, self.strength, alpha)


def tune_tables(tunes, sampling_rate, block_size):
    """The settings `ddsp_f0_tune` takes for `job_tunes`' list at the model's frame rate -> CPU tensors (mask (J,) int32, param
    (J, 3) fp64: a4, strength, alpha); a job without a tune is off: mask 0, (440, 0, 1)."""
    hop = float(block_size) / float(sampling_rate)
    settings = [(0, (440.0, 0.0, 1.0)) if t is None else t.setting(hop) for t in tunes]
    return (torch.tensor([m for m, _ in settings], dtype=torch.int32),
            torch.tensor([list(p) for _, p in settings], dtype=torch.float64).reshape(-1, 3))


class UnitIndex:
    """The stored units of one voice, for unit retrieval (include/ddsp_amd.h states the rule at `ddsp_units_retrieve`): vectors
    (N, C) fp32 on the host, N >= 1, C a multiple of 4 and at most 1024, every value finite.  An index is the aligned units of a
    speaker's training files (`from_units_dir`); a large one is reduced to k-means centres on the device before it is served
    (`reduce`, `from_units_dir(centres=)`; include/ddsp_amd.h states that rule at `ddsp_units_kmeans_assign`).  IVF or any other
    approximate search is not here."""

    def __init__(self, vectors):
        v = torch.as_tensor(np.asarray(vectors) if not isinstance(vectors, torch.Tensor) else vectors)
        if not (v.dim() == 2 and v.shape[0] >= 1 and 4 <= v.shape[1] <= 1024 and v.shape[1] % 4 == 0 and v.is_floating_point()):
            raise ValueError(f"UnitIndex: vectors must be (N, C) floating point with N >= 1 and C a multiple of 4 in 4..1024, got "
                             f"{tuple(v.shape)} {v.dtype}")
        v = v.detach().to("cpu", torch.float32).contiguous()
        if not bool(torch.isfinite(v).all()):
            raise ValueError("UnitIndex: vectors must be finite")
        self.vectors = v

    def __len__(self):
        return int(self.vectors.shape[0])

    @property
    def channels(self):
        return int(self.vectors.shape[1])

    @staticmethod
    def fixed_shift(vectors):
        """S = 62 - E - L of the reduction's fixed point: max|vectors| < 2^E (the frexp exponent; 0 for an all-zero index) and
        L = (N - 1).bit_length(), so the int64 sum of N values rint(x * 2^S) stays within 2^62."""
        top = float(vectors.abs().max())
        return 62 - (math.frexp(top)[1] if top > 0 else 0) - (int(vectors.shape[0]) - 1).bit_length()

    def reduce(self, centres, iters=10, device="cuda", report=False):
        """The index reduced to at most `centres` k-means centres on `device` (include/ddsp_amd.h states the rule at
        `ddsp_units_kmeans_assign`; it is deterministic): the centres start as the `max_entries` subset, `iters` full Lloyd
        iterations of (`ddsp_units_index_norms`, `ddsp_units_kmeans_assign`, `ddsp_units_kmeans_update`) run on one stream with
        no read-back between them, and the centres that hold entries in the last iteration are kept, in id order.  One upload,
        one read-back.  `centres >= len(self)`: self, unchanged.  report=True -> (index, {"moved": entries that changed centre in
        every iteration, "count": (K,) int32 entries of every centre in the last one, "dropped": the empty centres left out,
        "shift": the fixed point's S}).  ValueError for a `centres` that is no int >= 1 or an `iters` that is no int >= 0."""
        if isinstance(centres, bool) or not isinstance(centres, numbers.Integral) or centres < 1:
            raise ValueError(f"UnitIndex.reduce: centres must be an int >= 1, got {centres!r}")
        if isinstance(iters, bool) or not isinstance(iters, numbers.Integral) or iters < 0:
            raise ValueError(f"UnitIndex.reduce: iters must be an int >= 0, got {iters!r}")
        N, K, iters = len(self), int(centres), int(iters)
        shift = self.fixed_shift(self.vectors)
        if K >= N:
            rep = {"moved": [], "count": np.ones(N, dtype=np.int32), "dropped": 0, "shift": shift}
            return (self, rep) if report else self
        start = self.vectors[(torch.arange(K, dtype=torch.int64) * N) // K]
        if iters == 0:
            rep = {"moved": [], "count": np.ones(K, dtype=np.int32), "dropped": 0, "shift": shift}
            return (UnitIndex(start), rep) if report else UnitIndex(start)
        dev = torch.device(device)
        ctx = hipddsp.context_for(dev)                      # (refuses a device that is no HIP device)
        vec = self.vectors.to(dev)
        cen = start.to(dev)
        assign = torch.full((N,), -1, dtype=torch.int32, device=dev)
        moved = torch.zeros(iters, dtype=torch.int32, device=dev)
        count = torch.empty(K, dtype=torch.int32, device=dev)
        ws = torch.empty(K * self.channels, dtype=torch.int64, device=dev)
        for it in range(iters):
            cnrm = ctx.units_index_norms(cen)
            ctx.units_kmeans_assign_(vec, cen, cnrm, assign, moved[it:it + 1])
            ctx.units_kmeans_update_(vec, assign, cen, count, shift, ws)
        back = torch.cat([cen.view(torch.int32).reshape(-1), count, moved]).cpu()                  # the one read-back
        cen_h = back[:K * self.channels].view(torch.float32).reshape(K, self.channels)
        count_h = back[K * self.channels:K * self.channels + K]
        out = UnitIndex(cen_h[count_h > 0])
        if not report:
            return out
        return out, {"moved": back[K * self.channels + K:].tolist(), "count": count_h.numpy().copy(),
                     "dropped": int((count_h == 0).sum()), "shift": shift}

    @classmethod
    def from_units_dir(cls, path, spk=None, max_entries=None, centres=None, iters=10, device="cuda"):
        """The index of the `units/` tree that `preprocess.py` wrote under `path` (<path>/units/<spk>/<name>.0.npy, each (n, C)):
        every file of speaker folder `spk` (None: of all folders), sorted by relative name, frame after frame.  max_entries: a
        deterministic evenly strided subset of that many rows (row floor(i * N / max_entries)) when there are more.  centres: the
        rows - what max_entries left of them - are then reduced to that many k-means centres by `reduce(centres, iters, device)`."""
        for name, v, low in (("centres", centres, 1), ("iters", iters, 0)):
            if (v is not None or name == "iters") and (isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < low):
                raise ValueError(f"UnitIndex.from_units_dir: {name} must be an int >= {low}, got {v!r}")
        root = os.path.join(path, "units")
        if spk is not None:
            root = os.path.join(root, str(spk))
        names = sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs if f.endswith(".npy"))
        if not names:
            raise ValueError(f"UnitIndex.from_units_dir: no .npy under {root}")
        files = [np.load(os.path.join(root, n)) for n in names]
        rows = np.concatenate([f.astype(np.float32).reshape(-1, f.shape[-1]) for f in files])
        if max_entries is not None:
            if isinstance(max_entries, bool) or not isinstance(max_entries, numbers.Integral) or max_entries < 1:
                raise ValueError(f"UnitIndex.from_units_dir: max_entries must be an int >= 1, got {max_entries!r}")
            if len(rows) > max_entries:
                rows = rows[(np.arange(int(max_entries), dtype=np.int64) * len(rows)) // int(max_entries)]
        index = cls(rows)
        return index if centres is None else index.reduce(centres, iters=iters, device=device)

    def save(self, path):
        """A plain tensor file: torch.save of {'vectors': (N, C) fp32}."""
        torch.save({"vectors": self.vectors}, path)

    @classmethod
    def load(cls, path):
        d = torch.load(path, map_location="cpu", weights_only=True)
        if not (isinstance(d, dict) and isinstance(d.get("vectors"), torch.Tensor)):
            raise ValueError(f"UnitIndex.load: {path} holds no {{'vectors': tensor}}")
        return cls(d["vectors"])


class UnitIndexBank:
    """X indices in one device arena, as `ddsp_units_retrieve` takes them: off (X + 1,) int64 row offsets, vec (N_total, C)
    fp32, nrm (N_total,) fp32 (formed once here by `ddsp_units_index_norms`), `n_max` the largest N.  The workspace of the
    search is the bank's: allocated here for calls of up to `rows` rows of `frames` frames at `k` neighbours - the size
    `ddsp_units_retrieve_workspace` gives grows with the rows, so every call of fewer rows is served too -, and `workspace(rows,
    Fr, k)` refuses a larger call (nothing is allocated at a launch; `reserve` grows it outside a capture).
    ONE STREAM AT A TIME: the one workspace is written by every `units_retrieve_` call through this bank, so two consumers that
    launch on different streams - two StreamBanks, or a StreamBank and an offline render - race on it; give each a
    `UnitIndexBank` of its own (the vectors are the `UnitIndex`'s and are not copied on the host).
    ValueError for an empty list, an entry that is no `UnitIndex`, or indices of different widths."""

    def __init__(self, indices, device="cuda", rows=16, frames=256, k=8):
        indices = list(indices) if isinstance(indices, (list, tuple)) else None
        if not indices or not all(isinstance(i, UnitIndex) for i in indices):
            raise ValueError("UnitIndexBank: indices must be a non-empty list of UnitIndex")
        if len({i.channels for i in indices}) != 1:
            raise ValueError(f"UnitIndexBank: the indices of a bank agree in width, got {[i.channels for i in indices]}")
        for name, v in (("rows", rows), ("frames", frames)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
                raise ValueError(f"UnitIndexBank: {name} must be an int >= 1, got {v!r}")
        if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= k <= hipddsp.MAX_RETRIEVE_K:
            raise ValueError(f"UnitIndexBank: k must be an int in 1..{hipddsp.MAX_RETRIEVE_K}, got {k!r}")
        self.sizes = [len(i) for i in indices]
        self.n_max, self.channels = max(self.sizes), indices[0].channels
        self.device = torch.device(device)
        ctx = hipddsp.context_for(self.device)              # (refuses a device that is no HIP device)
        self.off = torch.tensor(np.concatenate([[0], np.cumsum(self.sizes)]), dtype=torch.int64).to(self.device)
        self.vec = torch.cat([i.vectors for i in indices]).to(self.device).contiguous()
        self.device = self.vec.device                       # (with its number: 'cuda' is 'cuda:0' here)
        self.nrm = ctx.units_index_norms(self.vec)
        self._ctx = ctx
        self._ws = None
        self.reserve(rows, frames, k)

    def __len__(self):
        return len(self.sizes)

    def reserve(self, rows, frames, k):
        """Grow the workspace to serve calls of rows x frames queries at k neighbours (an allocation: never inside a capture)."""
        need = max(self._ctx.units_retrieve_workspace(int(rows), int(frames), int(k), self.n_max), 8)
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = torch.empty((need + 3) // 4, dtype=torch.int32, device=self.device)

    def workspace(self, rows, Fr, k):
        need = self._ctx.units_retrieve_workspace(rows, Fr, k, self.n_max)
        if self._ws.numel() * 4 < need:
            raise ValueError(f"UnitIndexBank: a call of {rows} x {Fr} frames at k = {k} needs a workspace of {need} bytes, this bank "
                             f"holds {self._ws.numel() * 4}: `reserve(rows, frames, k)` outside any capture")
        return self._ws


def index_tables(settings):
    """`job_indices`' list -> CPU tensors (index_of_job (J,) int32, -1 for a job without one; ratio_of_job (J,) fp32, 0 there)."""
    return (torch.tensor([-1 if s is None else int(s[0]) for s in settings], dtype=torch.int32),
            torch.tensor([0.0 if s is None else float(s[1]) for s in settings], dtype=torch.float32))


def check_job_index(who, setting, n_indices=None):
    """A job's seventh entry: None or (index_number, ratio) with an int >= 0 (and < n_indices where the bank is known) and a
    finite ratio in [0, 1]; ValueError otherwise."""
    if setting is None:
        return
    ok = isinstance(setting, (tuple, list)) and len(setting) == 2
    if ok:
        i, r = setting
        ok = isinstance(i, numbers.Integral) and not isinstance(i, bool) and i >= 0 and (n_indices is None or i < n_indices) and \
            isinstance(r, numbers.Real) and not isinstance(r, bool) and math.isfinite(r) and 0 <= r <= 1
    if not ok:
        bank = "" if n_indices is None else f" of the {n_indices} indices of the call"
        raise ValueError(f"{who}: index must be None or (index_number, ratio) with index_number >= 0{bank} and ratio in [0, 1], "
                         f"got {setting!r}")


class EnvelopeMix:
    """The envelope mix of a job (its eighth entry) or of a bank's slot: the converted output is held to the SOURCE's loudness
    envelope - RVC's `rms_mix_rate` (`change_rms`), so-vits-svc's "loudness envelope adjustment"; include/ddsp_amd.h states the
    rule at `ddsp_envelope_rms`.  rate in [0, 1]: the share of the output's OWN envelope that is kept - 1 changes nothing, 0
    gives the output the source's envelope.  hop_seconds > 0: the distance of the RMS frames (RVC: half a second offline, 10 ms
    live); frames: the window in hops, 2, 4, 6 or 8 (RVC: 2 offline, 4 live).  A silent source silences the output (the gain
    is e1^(1 - rate) * e2^(rate - 1), and e1 is 0 there), as in RVC.  ValueError for anything else."""

    def __init__(self, rate, hop_seconds=0.5, frames=2):
        def real(x):
            return isinstance(x, numbers.Real) and not isinstance(x, bool) and math.isfinite(x)
        if not (real(rate) and 0 <= rate <= 1):
            raise ValueError(f"EnvelopeMix: rate must be a number in [0, 1], got {rate!r}")
        if not (real(hop_seconds) and hop_seconds > 0):
            raise ValueError(f"EnvelopeMix: hop_seconds must be a finite number of seconds > 0, got {hop_seconds!r}")
        if isinstance(frames, bool) or not isinstance(frames, numbers.Integral) or frames not in (2, 4, 6, 8):
            raise ValueError(f"EnvelopeMix: frames must be 2, 4, 6 or 8 (the window in hops), got {frames!r}")
        self.rate, self.hop_seconds, self.frames = float(rate), float(hop_seconds), int(frames)

    def setting(self, sr):
        """-> the hop in samples at `sr` Hz, int(sr * hop_seconds): RVC's sr // 2 at the default.  ValueError for a rate at
        which the hop is no sample long."""
        if not (isinstance(sr, numbers.Real) and not isinstance(sr, bool) and math.isfinite(sr) and sr > 0):
            raise ValueError(f"EnvelopeMix.setting: sr must be a finite number of Hz > 0, got {sr!r}")
        hop = int(sr * self.hop_seconds)
        if not 1 <= hop <= 2 ** 27:
            raise ValueError(f"EnvelopeMix.setting: a hop of {self.hop_seconds} s at {sr} Hz is {hop} samples, outside 1..2**27")
        return hop


def envelope_tables(envelopes):
    """`job_envelopes`' list -> (rate (J,) fp64 CPU tensor - 1, which is off, for a job without one -, hop_seconds, frames),
    the last two None when no job has one.  All jobs of a call share `hop_seconds` and `frames` (one RMS launch serves them)
    and differ in `rate`: ValueError for two that disagree."""
    given = [e for e in envelopes if e is not None]
    shape = {(e.hop_seconds, e.frames) for e in given}
    if len(shape) > 1:
        raise ValueError(f"envelope_tables: the jobs of one call share hop_seconds and frames and differ in rate, got "
                         f"{sorted(shape)}")
    rate = torch.tensor([1.0 if e is None else e.rate for e in envelopes], dtype=torch.float64)
    return (rate, *(next(iter(shape)) if shape else (None, None)))


@dataclasses.dataclass
class Job:
    """One offline job by name: a file and a model (their numbers in the call), a speaker (an id, a mix dict or a
    `SpeakerTimeline`), a key (semitones or a `KeyTimeline`) and the controls it carries, None for one it does not: formant
    (semitones or a `FormantTimeline`), tune (a `PitchTune`), index ((index_number, ratio) into the call's `UnitIndexBank`) and
    envelope (an `EnvelopeMix`).  `infer_offline.job_table` states and checks the values."""
    file: object
    model: object
    spk: object
    key: object
    formant: object = None
    tune: object = None
    index: object = None
    envelope: object = None

    @classmethod
    def of(cls, j, job, who="job_table"):
        """Job `j` of a call as a `Job`: a `Job` as it is, or the positional form - a tuple or list of the first four to eight
        fields in the order above, a sixth that is None or a `PitchTune`, an eighth that is an `EnvelopeMix` itself (a tuple
        WITHOUT the envelope is the shorter tuple: eight entries ending in None stay refused, as every 8-tuple was before the
        control; a record simply leaves the field None).  ValueError in the name of `who` otherwise."""
        if isinstance(job, cls):
            return job
        if not (isinstance(job, (tuple, list)) and len(job) in (4, 5, 6, 7, 8) and (len(job) < 6 or job[5] is None or
                                                                                   isinstance(job[5], PitchTune)) and
                (len(job) < 8 or job[7] is not None)):
            raise ValueError(f"{who}: job {j} must be (file, model_index, spk, key), (file, model_index, spk, key, formant) or "
                             f"(file, model_index, spk, key, formant, tune) with tune a PitchTune or None, or those six with "
                             f"(index_number, ratio) or None behind them, or those seven with an EnvelopeMix behind them "
                             f"(a job without one is the shorter tuple), got {job!r}")
        if len(job) == 8 and not isinstance(job[7], EnvelopeMix):
            raise ValueError(f"{who}: job {j}: envelope must be an EnvelopeMix, got {job[7]!r}")
        return cls(*job)


def job_formants(jobs):
    """The formant shift of every job of a `job_table` call, in job order: None, a float of semitones or the `FormantTimeline`
    as it is.  `job_table` has checked them."""
    formants = (Job.of(j, job).formant for j, job in enumerate(jobs))
    return [f if f is None or isinstance(f, FormantTimeline) else float(f) for f in formants]


def job_tunes(jobs):
    """The pitch correction of every job of a `job_table` call, in job order: its `PitchTune`, else None."""
    return [Job.of(j, job).tune for j, job in enumerate(jobs)]


def job_indices(jobs):
    """The retrieval setting of every job of a `job_table` call, in job order: its (index_number, ratio), else None."""
    return [Job.of(j, job).index for j, job in enumerate(jobs)]


def job_envelopes(jobs):
    """The envelope mix of every job of a `job_table` call, in job order: its `EnvelopeMix`, else None."""
    return [Job.of(j, job).envelope for j, job in enumerate(jobs)]
