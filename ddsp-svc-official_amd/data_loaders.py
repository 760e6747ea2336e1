"""The reference's `data_loaders.py` (`AudioDataset`, `get_data_loaders`) on the device path.

The reference caches every file as its own tensors and builds a batch from B `__getitem__` calls (about four slices each)
and five `torch.stack` collations.  Here the dataset `preprocess.py` wrote is packed ONCE into arenas on the device - audio
back to back, (n_aunit + 1) units arenas, f0 and volume, with per-file tables - and a batch is ONE launch
(`ddsp_dataset_gather`): row b is the triple (file, start_frame, unit_idx), injected by the caller or drawn in the kernel
from a device permutation, a cursor and a seed, so nothing is read back and nothing synchronises.

The host part is plain numpy and needs neither a GPU nor the shared library: `list_stems`, `scan_tree`, `pack_arenas`,
`next_valid_table`, `start_frame`, `crop_frames`, `whole_frames`, `epoch_plan`.  `AudioDataset` calls them and uploads.

What differs from the reference, all of it additive:
  * files are listed sorted, as `preprocess.list_audio` does (the reference keeps os.walk's order, the file system's);
  * an fp16 cache (`fp16=True`) still yields fp32 tensors - the same values, promoted on the way out;
  * a file whose f0 / volume / units / audio are shorter than its longest possible crop is refused by name when the dataset
    is built (in the reference the slice comes out short and the collation fails later);
  * `load_all_data=False` and `device='cpu'` raise: there is no CPU path.
"""
import os

import numpy as np

from infer_offline import group_segments
from preprocess import list_audio, load_wav
from sharding import RaggedPlan, shard_rows

AUDIO_ALIGN = 8     # elements: every file's first sample sits on 16 bytes in an fp32 and in an fp16 arena
ARENA_ALIGN = 8     # total_frames * n_unit is a multiple of it: every units arena starts on 16 bytes


# ---- host part (numpy only) ---------------------------------------------------------------------------------------------
def list_stems(path_root):
    """`<path_root>/audio/**/*.wav` as stems relative to audio/ ("5/uttr_001"), sorted."""
    return [os.path.splitext(rel)[0] for rel in list_audio(os.path.join(path_root, "audio"))]


def frame_sec(hop_size, sample_rate):
    """The reference's `frame_resolution` (`data_loaders.py:125`)."""
    return hop_size / sample_rate


def crop_frames(waveform_sec, hop_size, sample_rate):
    """Frames of a cropped item: `int(waveform_sec / frame_resolution)` (`data_loaders.py:130`)."""
    return int(waveform_sec / frame_sec(hop_size, sample_rate))


def whole_frames(duration, hop_size, sample_rate):
    """Frames of a whole-audio item: the same formula with the file's own duration (`data_loaders.py:127,130`)."""
    return int(duration / frame_sec(hop_size, sample_rate))


def start_frame(u, duration, waveform_sec, hop_size, sample_rate):
    """The start frame of a crop from u in [0, 1): `random.uniform(0, duration - waveform_sec - 0.1)` is `hi * u`, then
    `int(idx_from / frame_resolution)` (`data_loaders.py:128-129`), in fp64 as Python evaluates it - and as the kernel does."""
    return int((u * (duration - waveform_sec - 0.1)) / frame_sec(hop_size, sample_rate))


def max_start_frame(duration, waveform_sec, hop_size, sample_rate):
    """The largest start frame any u < 1 can give."""
    return start_frame(1.0, duration, waveform_sec, hop_size, sample_rate)


def next_valid_table(durations, waveform_sec):
    """next_valid[i]: the first file at or cyclically after i with duration >= waveform_sec + 0.1 - where the reference's
    `__getitem__` ends up after its skips (`data_loaders.py:92-93`); -1 everywhere when no file is long enough."""
    d = np.asarray(durations, dtype=np.float64)
    n = len(d)
    ok = ~(d < (waveform_sec + 0.1))
    out = np.full(n, -1, dtype=np.int32)
    if not ok.any():
        return out
    nxt = -1
    for i in list(range(n - 1, -1, -1)) * 2:      # twice round, backwards: the second pass fills the wrap-around
        if ok[i]:
            nxt = i
        out[i] = nxt
    return out


def scan_tree(path_root, sample_rate, n_spk=1, n_aunit=0, load=None):
    """Reads the tree `preprocess.py` wrote: -> a list of records {name, audio (T,) float32, duration, f0 (n,), volume (n,),
    units [(n, C)] * (n_aunit + 1), spk_id}, in `list_stems` order, with the reference's checks (`data_loaders.py:57-78`): the
    speaker directory is a digit string, the id is within [1, n_spk], the f0 / volume / units files exist.  A wav at another
    rate than `sample_rate` raises ValueError (`preprocess` has written the tree at the model's rate).  duration is
    samples / rate, what `librosa.get_duration` gives for such a file."""
    load = load_wav if load is None else load
    records = []
    for stem in list_stems(path_root):
        spk_name = os.path.dirname(stem)
        if not str.isdigit(spk_name):
            raise ValueError(f"{stem}: the speaker directory must be a positive integer, got '{spk_name}'")
        spk_id = int(spk_name)
        if spk_id < 1 or n_spk < spk_id:
            raise ValueError(f"{stem}: spk_id (the directory name) must be within [1, n_spk = {n_spk}]")
        paths = {"f0": os.path.join(path_root, "f0", stem) + ".npy", "volume": os.path.join(path_root, "volume", stem) + ".npy"}
        paths.update({f"units.{k}": os.path.join(path_root, "units", stem) + f".{k}.npy" for k in range(1 + int(n_aunit))})
        for what, p in paths.items():
            if not os.path.isfile(p):
                raise FileNotFoundError(f"{stem}: the {what} file {p} is missing")
        audio, rate = load(os.path.join(path_root, "audio", stem) + ".wav")
        if int(rate) != int(sample_rate):
            raise ValueError(f"{stem}: the wav is at {int(rate)} Hz, the dataset at {int(sample_rate)} Hz (preprocess writes "
                             "the tree at the model's rate; files are not resampled here)")
        audio = np.ascontiguousarray(audio, dtype=np.float32).reshape(-1)
        records.append({
            "name": stem, "audio": audio, "duration": len(audio) / int(sample_rate), "spk_id": spk_id,
            "f0": np.load(paths["f0"]).astype(np.float32).reshape(-1),
            "volume": np.load(paths["volume"]).astype(np.float32).reshape(-1),
            "units": [np.load(paths[f"units.{k}"]).astype(np.float32) for k in range(1 + int(n_aunit))],
        })
    return records


def check_lengths(records, waveform_sec, hop_size, sample_rate, whole_audio=False):
    """Every file must hold its longest possible crop: in whole-audio mode `whole_frames(duration)` frames from 0; else,
    for a file the skip lets through, `crop_frames` frames from its largest start frame - in f0, volume, every units copy
    and (times hop_size) the audio.  ValueError names the first file that does not; a whole file of less than 1 frame too."""
    crop = crop_frames(waveform_sec, hop_size, sample_rate)
    for r in records:
        if whole_audio:
            need = whole_frames(r["duration"], hop_size, sample_rate)
            if need < 1:
                raise ValueError(f"{r['name']}: {len(r['audio'])} samples are less than one frame of {hop_size}")
        elif r["duration"] < waveform_sec + 0.1:
            continue
        else:
            need = max_start_frame(r["duration"], waveform_sec, hop_size, sample_rate) + crop
        have = min([len(r["f0"]), len(r["volume"]), len(r["audio"]) // hop_size] + [u.shape[0] for u in r["units"]])
        if have < need:
            raise ValueError(f"{r['name']}: its longest crop needs {need} frames but f0 / volume / units / audio hold {have}")


def pack_arenas(records, waveform_sec, fp16=False):
    """records (`scan_tree`) -> (arenas, tables), numpy, laid out as `ddsp_dataset_view` (include/ddsp_amd.h) wants them:
    arenas: audio (sum of the padded lengths,) and units (n_aunit + 1, total_frames, C) in fp32 or fp16, f0 and volume
            (total_frames,) fp32; every file's audio starts on a multiple of 8 elements and total_frames * C is a multiple of
            8 (16 bytes in either type), the padding is zeros;
    tables: audio_off, audio_len, frame_off (int64), frames (int32: the rows every frame series of the file holds), spk_id
            (int64), duration (float64), next_valid (int32)."""
    n = len(records)
    if n == 0:
        raise ValueError("the dataset holds no file")
    C = int(records[0]["units"][0].shape[1])
    n_copies = len(records[0]["units"])
    for r in records:
        for u in r["units"]:
            if u.ndim != 2 or u.shape[1] != C:
                raise ValueError(f"{r['name']}: units of shape {u.shape}, the dataset's are (frames, {C})")
    frames = np.array([min([len(r["f0"]), len(r["volume"])] + [u.shape[0] for u in r["units"]]) for r in records], dtype=np.int32)
    audio_len = np.array([len(r["audio"]) for r in records], dtype=np.int64)
    padded = (audio_len + AUDIO_ALIGN - 1) // AUDIO_ALIGN * AUDIO_ALIGN
    audio_off = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
    frame_off = np.concatenate([[0], np.cumsum(frames.astype(np.int64))[:-1]]).astype(np.int64)
    total_frames = max(int(frames.astype(np.int64).sum()), 1)
    while (total_frames * C) % ARENA_ALIGN:
        total_frames += 1
    dt = np.float16 if fp16 else np.float32
    audio = np.zeros(max(int(padded.sum()), AUDIO_ALIGN), dtype=dt)
    units = np.zeros((n_copies, total_frames, C), dtype=dt)
    f0 = np.zeros(total_frames, dtype=np.float32)
    volume = np.zeros(total_frames, dtype=np.float32)
    for i, r in enumerate(records):
        a0, f_lo, nf = int(audio_off[i]), int(frame_off[i]), int(frames[i])
        audio[a0:a0 + len(r["audio"])] = r["audio"]
        f0[f_lo:f_lo + nf] = r["f0"][:nf]
        volume[f_lo:f_lo + nf] = r["volume"][:nf]
        for k, u in enumerate(r["units"]):
            units[k, f_lo:f_lo + nf] = u[:nf]
    duration = np.array([r["duration"] for r in records], dtype=np.float64)
    tables = {"audio_off": audio_off, "audio_len": audio_len, "frame_off": frame_off, "frames": frames,
              "spk_id": np.array([r["spk_id"] for r in records], dtype=np.int64), "duration": duration,
              "next_valid": next_valid_table(duration, waveform_sec)}
    return {"audio": audio, "units": units, "f0": f0, "volume": volume}, tables


def epoch_plan(n_files, batch_size, rank=0, world=1, even=False):
    """What `DataLoader(shuffle=True)` does with one permutation of the files: [(cursor, rows)] per step - the global batch
    at [start, start + size) of the permutation, the last one shorter (no drop_last), of which `rank` takes its
    `sharding.shard_rows` slice: `rows` rows from permutation index `cursor` on (rows may be 0 in a short last batch).
    even: a global batch keeps the largest multiple of `world` rows it holds (the training loop's form: equal shards, whose
    mean loss is the global loss, and the same number of steps on every rank); a batch of fewer than `world` rows is left
    out on every rank."""
    if batch_size < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"epoch_plan: batch_size {batch_size}, rank {rank} of {world}")
    plan = []
    for start in range(0, int(n_files), int(batch_size)):
        size = min(int(batch_size), int(n_files) - start)
        if even:
            size -= size % world
            if size == 0:
                continue
        lo, hi = shard_rows(size, world, rank)
        plan.append((start + lo, hi - lo))
    return plan


def shard_whole(n_frames, rank, world):
    """The rows (indices into `n_frames`) of a global group of whole utterances that `rank` trains on: the balanced deal of
    `sharding.RaggedPlan`.  Over the ranks the lists are a partition of the group."""
    return RaggedPlan(n_frames, world).local(rank)


def epoch_seed(seed, epoch):
    """The seed of one epoch's permutation and draws (the same on every rank)."""
    return (int(seed) * 0x9E3779B97F4A7C15 + int(epoch) * 0xD1B54A32D192ED03 + 0x2545F4914F6CDD1D) & ((1 << 63) - 1)


# ---- device part --------------------------------------------------------------------------------------------------------
class AudioDataset:
    """The reference's `AudioDataset` (`data_loaders.py:27`) with the dataset resident on the device in packed arenas.

    `batch` / `batches` / `whole_batches` produce what `training.train_step` takes, one kernel launch each; `__getitem__` is
    the reference's per-file dict through the same kernel at B = 1 (the compatibility path, not the fast one)."""

    def __init__(self, path_root, waveform_sec, hop_size, sample_rate, load_all_data=True, whole_audio=False, n_spk=1,
                 n_aunit=0, device="cuda", fp16=False, records=None):
        """The reference's arguments; `records`: file records as `scan_tree` returns them, in place of reading `path_root`
        (a dataset that is already in memory)."""
        import torch
        if not load_all_data:
            raise ValueError("AudioDataset: load_all_data=False (streaming from disk) is not supported - the dataset lives on "
                             "the device")
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"AudioDataset: device={device!r} - the dataset lives on a HIP device (no CPU path)")
        self.path_root, self.waveform_sec, self.hop_size, self.sample_rate = path_root, waveform_sec, int(hop_size), int(sample_rate)
        self.whole_audio, self.n_spk, self._n_aunit, self.fp16 = bool(whole_audio), int(n_spk), int(n_aunit), bool(fp16)
        records = scan_tree(path_root, sample_rate, n_spk, n_aunit) if records is None else records
        if not records:
            raise ValueError(f"AudioDataset: no wav under {os.path.join(path_root, 'audio')}")
        check_lengths(records, waveform_sec, hop_size, sample_rate, whole_audio)
        self.paths = [r["name"] for r in records]
        arenas, tables = pack_arenas(records, waveform_sec, fp16)
        self.duration = tables["duration"]
        self._frames, self._audio_len = tables["frames"], tables["audio_len"]
        self.next_valid = tables["next_valid"]
        self.spk_ids = [int(v) for v in tables["spk_id"]]      # per file, on the host (validation names its speakers)
        self.crop = crop_frames(waveform_sec, hop_size, sample_rate)
        self.whole = [whole_frames(d, hop_size, sample_rate) for d in self.duration]
        self._upload(arenas, tables, device)
        self._epoch = 0
        self._rng = np.random.default_rng()

    def _upload(self, arenas, tables, device):
        import torch
        import hipddsp
        self.ctx = hipddsp.context_for(torch.device(device))
        self.device = self.ctx.device
        self._dev = {k: torch.from_numpy(v).to(self.device) for k, v in {**arenas, **tables}.items()}
        units = self._dev["units"]
        self.view = hipddsp.DatasetView(
            **{k: self._dev[k].data_ptr() for k in ("audio", "units", "f0", "volume", "audio_off", "audio_len", "frame_off",
                                                    "frames", "spk_id", "duration", "next_valid")},
            n_files=len(self.paths), total_frames=units.shape[1], n_aunit=self._n_aunit, n_unit=units.shape[2],
            hop=self.hop_size, sample_rate=self.sample_rate, fp16=1 if self.fp16 else 0)

    def __len__(self):
        return len(self.paths)

    # -- batches ----------------------------------------------------------------------------------------------------------
    def _triples(self, triples):
        import torch
        if not isinstance(triples, torch.Tensor):
            triples = torch.as_tensor(np.asarray(triples, dtype=np.int32).reshape(-1, 3))
        return triples.to(device=self.device, dtype=torch.int32).contiguous()

    def _finish(self, out, n_frames=None):
        batch = {k: out[k] for k in ("units", "f0", "volume", "spk_id", "audio", "draws")}
        if n_frames is not None:
            batch["n_frames"] = n_frames
        return batch

    def batch(self, triples=None, *, batch_size=None, seed=None, perm=None, cursor=0, out=None):
        """One cropped batch: the dict `training.train_step` takes (units (B,Fr,C), f0 (B,Fr,1), volume (B,Fr), spk_id (B,1),
        audio (B,Fr*hop), Fr = `crop_frames`), plus `draws` (the (B,3) int32 device tensor of the (file, start_frame,
        unit_idx) used) and `name` (a list; reading it copies `draws` to the host, so it is made on first access).
        triples: (B,3) ints, injected - the parity form, like `noise=` on the synthesisers.  Otherwise the batch is DRAWN
        in the kernel: `batch_size` rows from `perm` (a device int32 tensor of file indices, default: `batch_size` draws with
        replacement from `seed`) at `cursor`, crops and unit copies from counter hashes of (seed, cursor + row)."""
        import torch
        if triples is not None:
            t = self._triples(triples)
            got = self.ctx.dataset_gather(self.view, t.shape[0], max(self.crop, 1), triples=t, crop_frames=self.crop, out=out)
        else:
            if batch_size is None:
                raise ValueError("batch: pass triples or batch_size")
            if (self.next_valid < 0).any():
                raise ValueError(f"batch: no file is as long as waveform_sec + 0.1 = {self.waveform_sec + 0.1} s")
            seed = int(self._rng.integers(1 << 62)) if seed is None else int(seed)
            if perm is None:
                g = torch.Generator(device=self.device)
                g.manual_seed(seed)
                perm = torch.randint(len(self), (int(batch_size),), device=self.device, dtype=torch.int32, generator=g)
            got = self.ctx.dataset_gather(self.view, int(batch_size), max(self.crop, 1), perm=perm, cursor=cursor, seed=seed,
                                          crop_frames=self.crop, waveform_sec=self.waveform_sec, out=out)
        return _Batch(self._finish(got), self.paths)

    def batches(self, batch_size, seed=None, rank=0, world=1, epoch=None, even=False):
        """One epoch, as `DataLoader(shuffle=True)` walks it: a permutation of the files (made on the device with
        `torch.randperm`, nothing is synchronised), a batch per `batch_size` of it, the last one shorter.  Under data
        parallelism every rank passes the same `seed` and gets its `sharding.shard_rows` slice of each global batch.  Every
        call is a new epoch (a new permutation and new crops from the same `seed`); `epoch` names one instead of counting.
        `batch_size` is the GLOBAL batch; `even`: equal shards on every rank (`epoch_plan`)."""
        import torch
        if seed is None:
            if world > 1:
                raise ValueError("batches: the ranks of a data-parallel job must share a seed")
            seed = int(self._rng.integers(1 << 62))
        if epoch is None:
            epoch, self._epoch = self._epoch, self._epoch + 1
        s = epoch_seed(seed, epoch)
        g = torch.Generator(device=self.device)
        g.manual_seed(s)
        perm = torch.randperm(len(self), device=self.device, generator=g).to(torch.int32)
        for cursor, rows in epoch_plan(len(self), batch_size, rank, world, even):
            if rows:
                yield self.batch(batch_size=rows, seed=s, perm=perm, cursor=cursor)

    def whole_batch(self, files, unit_idx=None, out=None):
        """Whole utterances `files` (indices) as one padded batch with `n_frames` (a list): the ragged form `train_step` and
        the models take.  unit_idx: the units copy per row (default: drawn on the host, as the reference's random.randint)."""
        import torch
        files = [int(i) for i in files]
        n = [self.whole[i] for i in files]
        for i, k in zip(files, n):
            if k < 1:
                raise ValueError(f"{self.paths[i]}: a whole-audio row needs at least 1 frame")
            if k > self._frames[i] or k * self.hop_size > self._audio_len[i]:
                raise ValueError(f"{self.paths[i]}: the whole file is {k} frames but f0 / volume / units / audio hold fewer")
        if unit_idx is None:
            unit_idx = self._rng.integers(0, self._n_aunit + 1, size=len(files))
        t = self._triples([[i, 0, int(k)] for i, k in zip(files, unit_idx)])
        lens = torch.tensor(n, dtype=torch.int32).to(self.device)
        got = self.ctx.dataset_gather(self.view, len(files), max(n), triples=t, len_rows=lens, out=out)
        batch = _Batch(self._finish(got, n_frames=n), self.paths)
        batch["name"] = [self.paths[i] for i in files]         # the files were named by the caller: no copy of `draws`
        return batch

    def whole_groups(self, batch_frames):
        """Every file once, grouped with `infer_offline.group_segments` so that a group's padded size (rows * longest) stays
        within `batch_frames` frames -> the groups, lists of file indices (a pure function of the lengths: the same on
        every rank)."""
        for i, k in enumerate(self.whole):
            if k < 1:
                raise ValueError(f"{self.paths[i]}: a whole-audio row needs at least 1 frame")
        return group_segments(self.whole, int(batch_frames))

    def whole_batches(self, batch_frames, rank=0, world=1):
        """The groups of `whole_groups` as padded batches with `n_frames`.  Under data parallelism (`world > 1`) every rank
        walks the same global groups and gets its rows of each (`whole_shard`), with `global_n_frames`."""
        for group in self.whole_groups(batch_frames):
            batch = self.whole_batch(group) if world == 1 else self.whole_shard(group, rank, world)
            if batch is not None:
                yield batch

    def whole_shard(self, group, rank, world):
        """`rank`'s rows of the global group `group` (file indices): those `sharding.RaggedPlan(n_frames, world).local(rank)`
        names, as a ragged batch that also carries `global_n_frames`, the frame counts of the whole group in the group's
        order - the same list on every rank (`training.train_step` forms the loss's denominators from it).  A group of fewer
        than `world` rows would leave a rank without a row: None, on every rank."""
        n = [self.whole[i] for i in group]
        if len(group) < world:
            return None
        batch = self.whole_batch([group[j] for j in shard_whole(n, rank, world)])
        batch["global_n_frames"] = n
        return batch

    def __getitem__(self, file_idx):
        """The reference's item (`data_loaders.py:88-146`): the dict of one file - after the skip of a file shorter than
        waveform_sec + 0.1 - with a drawn crop (or the whole file with `whole_audio`), through the kernel at B = 1:
        audio (T,), f0 (Fr,1), volume (Fr,), units (Fr,C), spk_id (1,), name."""
        import torch
        if self.whole_audio:
            i = int(self.next_valid[int(file_idx) % len(self)])      # (the reference skips short files in this mode too)
            if i < 0:
                raise ValueError(f"no file is as long as waveform_sec + 0.1 = {self.waveform_sec + 0.1} s")
            b = self.whole_batch([i])
        else:
            perm = torch.tensor([int(file_idx) % len(self)], dtype=torch.int32).to(self.device)
            b = self.batch(batch_size=1, perm=perm)
        return dict(audio=b["audio"][0], f0=b["f0"][0], volume=b["volume"][0], units=b["units"][0], spk_id=b["spk_id"][0],
                    name=b["name"][0])


class _Batch(dict):
    """A batch dict whose `name` list is made when it is first asked for: the names follow from `draws`, which is on the
    device, and a training loop that never reads them never waits for the copy."""

    def __init__(self, tensors, paths):
        super().__init__(tensors)
        self._paths = paths

    def __missing__(self, key):
        if key != "name":
            raise KeyError(key)
        files = self["draws"][:, 0].tolist()
        self["name"] = [self._paths[i] if 0 <= i < len(self._paths) else None for i in files]
        return self["name"]

    def __contains__(self, key):
        return key == "name" or super().__contains__(key)


class _Loader:
    """An iterable over batches: every `iter()` is one pass (`make()` returns the iterator)."""

    def __init__(self, dataset, make):
        self.dataset, self._make = dataset, make

    def __iter__(self):
        return self._make()

    def __len__(self):
        return self._len() if hasattr(self, "_len") else len(self.dataset)


def get_data_loaders(args, whole_audio=False, rank=0, world=1):
    """-> (train, valid) as the reference's `get_data_loaders` (`data_loaders.py:12-24`), each iterable over batches:
    train: `batches(args.train.batch_size)` over args.data.train_path (whole files at batch 1 with `whole_audio`);
    valid: whole files at batch 1, in file order, over args.data.valid_path.
    Data parallel (`world > 1`): `args.train.batch_size` is the GLOBAL batch and must divide by `world` (ValueError);
    `rank` gets its equal share of every global batch, permutation and crops from `args.train.seed` (default 0) on every
    rank.  With `whole_audio` every rank walks the same global groups of `args.train.val_batch_frames` padded frames
    (default `solver.VAL_BATCH_FRAMES`), longest first, and takes its rows of each with `global_n_frames`."""
    if world > 1 and not whole_audio and int(args.train.batch_size) % world:
        raise ValueError(f"train.batch_size = {args.train.batch_size} is the global batch: it must divide by the {world} ranks")
    common = dict(waveform_sec=args.data.duration, hop_size=args.data.block_size, sample_rate=args.data.sampling_rate,
                  n_spk=args.model.n_spk, n_aunit=args.data.n_aunit)
    data_train = AudioDataset(args.data.train_path, load_all_data=args.train.cache_all_data, whole_audio=whole_audio,
                              device=args.train.cache_device, fp16=args.train.cache_fp16, **common)
    data_valid = AudioDataset(args.data.valid_path, load_all_data=True, whole_audio=True, device=data_train.device, **common)

    def one_by_one(ds, shuffle):
        order = ds._rng.permutation(len(ds)) if shuffle else range(len(ds))
        return (ds.whole_batch([i]) for i in order)

    seed = int(args.train.seed or 0)
    if whole_audio and world > 1:
        frames = int(args.train.val_batch_frames or 8192)
        train = _Loader(data_train, lambda: data_train.whole_batches(frames, rank, world))
        train._len = lambda: sum(len(g) >= world for g in data_train.whole_groups(frames))
    elif whole_audio:
        train = _Loader(data_train, lambda: one_by_one(data_train, True))
    elif world > 1:
        train = _Loader(data_train, lambda: data_train.batches(args.train.batch_size, seed, rank, world, even=True))
        train._len = lambda: len(epoch_plan(len(data_train), int(args.train.batch_size), rank, world, even=True))
    else:
        train = _Loader(data_train, lambda: data_train.batches(args.train.batch_size))
        train._len = lambda: -(-len(data_train) // int(args.train.batch_size))
    valid = _Loader(data_valid, lambda: one_by_one(data_valid, False))
    return train, valid
