"""The host part of `data_loaders` - listing, packing, tables, the skip, the start-frame formula, the epoch plan and the
refusals - without a GPU and without the shared library.  The yardstick of the first half is tests/golden/dataset_ref.npz:
what the reference's own `AudioDataset` returned on the same tree (tests/golden/make_golden_dataset.py)."""
import os

import numpy as np
import pytest

import data_loaders as DL
import dataset_cases as DC
from conftest import GOLDEN


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "dataset_ref.npz"))


@pytest.fixture(scope="module")
def tree(g, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("dataset_fixture"))
    DC.write_tree(root, DC.fixture_files(g), int(g["sr"]))
    return root


@pytest.fixture(scope="module")
def records(g, tree):
    return DL.scan_tree(tree, int(g["sr"]), n_spk=int(g["n_spk"]), n_aunit=int(g["n_aunit"]))


def test_listing_order_and_contents(g, tree, records):
    assert DL.list_stems(tree) == [str(n) for n in g["names"]]
    assert [r["name"] for r in records] == [str(n) for n in g["names"]]
    for i, r in enumerate(records):
        assert np.array_equal(r["audio"], g[f"audio_{i}"].astype(np.float32) / 32768.0)
        assert np.array_equal(r["f0"], g[f"f0_{i}"]) and np.array_equal(r["volume"], g[f"volume_{i}"])
        assert r["spk_id"] == int(os.path.dirname(r["name"]))
        for k, u in enumerate(r["units"]):
            assert np.array_equal(u, g[f"units_{i}_{k}"])


def test_durations(g, records):
    assert np.array_equal(np.array([r["duration"] for r in records]), g["duration"])      # fp64, bit for bit


@pytest.mark.parametrize("mode", ["crop", "whole"])
def test_next_valid_reproduces_every_returned_name(g, records, mode):
    names = [str(n) for n in g["names"]]
    nv = DL.next_valid_table([r["duration"] for r in records], float(g["sec"]))
    assert nv.dtype == np.int32
    short = [i for i, r in enumerate(records) if r["duration"] < float(g["sec"]) + 0.1]
    assert len(short) >= 1 and len(names) - 1 in short                # a skip in the middle and one that wraps round
    for asked, name in zip(g[f"{mode}_asked"], g[f"{mode}_name"]):
        assert names[nv[int(asked)]] == str(name)
    assert set(int(a) for a in g[f"{mode}_asked"]) == set(range(len(names)))


def test_start_frame_formula(g, records):
    names = [str(n) for n in g["names"]]
    sec, hop, sr = float(g["sec"]), int(g["hop"]), int(g["sr"])
    for name, u, hi, idx_from, start in zip(g["crop_name"], g["crop_u"], g["crop_hi"], g["crop_idx_from"], g["crop_start"]):
        d = records[names.index(str(name))]["duration"]
        assert d - sec - 0.1 == hi and u * hi == idx_from             # the reference's own operands, bit for bit
        assert DL.start_frame(float(u), d, sec, hop, sr) == int(start)
        assert 0 <= int(start) <= DL.max_start_frame(d, sec, hop, sr)
    assert len(set(int(s) for s in g["crop_start"])) > 8


def test_crop_and_whole_lengths(g, records):
    names = [str(n) for n in g["names"]]
    sec, hop, sr = float(g["sec"]), int(g["hop"]), int(g["sr"])
    n = DL.crop_frames(sec, hop, sr)
    assert g["crop_f0"].shape[1:] == (n, 1) and g["crop_audio"].shape[1] == n * hop
    assert g["crop_units"].shape[1:] == (n, int(g["n_unit"])) and g["crop_volume"].shape[1] == n
    for j, name in enumerate(g["whole_name"]):
        k = DL.whole_frames(records[names.index(str(name))]["duration"], hop, sr)
        assert g[f"whole_f0_{j}"].shape == (k, 1) and g[f"whole_audio_{j}"].shape == (k * hop,)
        assert g[f"whole_units_{j}"].shape == (k, int(g["n_unit"])) and g[f"whole_volume_{j}"].shape == (k,)


def test_fixture_files_pass_the_length_check(g, records):
    DL.check_lengths(records, float(g["sec"]), int(g["hop"]), int(g["sr"]))
    DL.check_lengths(records, float(g["sec"]), int(g["hop"]), int(g["sr"]), whole_audio=True)


# ---- without the fixture ---------------------------------------------------------------------------------------------------
def _records(samples, hop=10, n_unit=3, n_aunit=1, sr=1000, extra_frames=1):
    names = [f"{1 + i % 2}/f{i}" for i in range(len(samples))]
    files = DC.make_files(names, samples, hop, n_unit, n_aunit, seed=5, extra_frames=extra_frames)
    return [{"name": f["name"], "audio": f["audio"].astype(np.float32) / 32768.0, "duration": len(f["audio"]) / sr,
             "spk_id": int(f["name"][0]), "f0": f["f0"], "volume": f["volume"], "units": f["units"]} for f in files]


@pytest.mark.parametrize("fp16", [False, True])
def test_table_dtypes_and_arena_padding(fp16):
    samples = [1003, 57, 700, 1, 333]
    recs = _records(samples)
    arenas, t = DL.pack_arenas(recs, 0.3, fp16=fp16)
    assert t["audio_off"].dtype == np.int64 and t["frame_off"].dtype == np.int64 and t["audio_len"].dtype == np.int64
    assert t["frames"].dtype == np.int32 and t["spk_id"].dtype == np.int64 and t["duration"].dtype == np.float64
    assert t["next_valid"].dtype == np.int32
    dt = np.float16 if fp16 else np.float32
    assert arenas["audio"].dtype == dt and arenas["units"].dtype == dt
    assert arenas["f0"].dtype == np.float32 and arenas["volume"].dtype == np.float32
    item = np.dtype(dt).itemsize
    assert all((int(o) * item) % 16 == 0 for o in t["audio_off"])                      # every file's audio starts on 16 bytes
    assert (arenas["units"].shape[1] * arenas["units"].shape[2] * item) % 16 == 0     # and so does every units arena
    assert arenas["units"].shape[0] == 2 and arenas["f0"].shape[0] == arenas["units"].shape[1]
    # files do not overlap, keep their order, and come back out of the arenas unchanged
    assert all(t["audio_off"][i] + t["audio_len"][i] <= t["audio_off"][i + 1] for i in range(len(recs) - 1))
    assert t["audio_off"][-1] + t["audio_len"][-1] <= arenas["audio"].shape[0]
    assert t["frame_off"][-1] + t["frames"][-1] <= arenas["f0"].shape[0]
    for i, r in enumerate(recs):
        a0, f_lo, nf = int(t["audio_off"][i]), int(t["frame_off"][i]), int(t["frames"][i])
        assert np.array_equal(arenas["audio"][a0:a0 + samples[i]], r["audio"].astype(dt))
        assert np.array_equal(arenas["f0"][f_lo:f_lo + nf], r["f0"]) and np.array_equal(arenas["volume"][f_lo:f_lo + nf], r["volume"])
        for k in range(2):
            assert np.array_equal(arenas["units"][k, f_lo:f_lo + nf], r["units"][k].astype(dt))
    assert list(t["next_valid"]) == [0, 2, 2, 0, 0]          # 0.3 + 0.1 s: files 0 and 2 pass; 3 and 4 wrap round to 0


def test_offsets_stay_int64_past_2_31():
    """Ten hours at 44.1 kHz are near 2^31 samples: the offsets are sums in int64 (formed here without the arena)."""
    lens = np.full(40, 60_000_000, dtype=np.int64)
    padded = (lens + DL.AUDIO_ALIGN - 1) // DL.AUDIO_ALIGN * DL.AUDIO_ALIGN
    off = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
    assert off[-1] > 2 ** 31 and off.dtype == np.int64


def test_next_valid_table_cases():
    assert list(DL.next_valid_table([1.0, 0.1, 0.1, 1.0], 0.5)) == [0, 3, 3, 3]
    assert list(DL.next_valid_table([0.1, 1.0, 0.1], 0.5)) == [1, 1, 1]
    assert list(DL.next_valid_table([0.1, 0.2], 0.5)) == [-1, -1]
    assert list(DL.next_valid_table([0.6], 0.5)) == [0]            # duration < sec + 0.1 skips; equal does not


@pytest.mark.parametrize("n_files,batch,world", [(6, 4, 1), (10, 4, 2), (7, 3, 3), (5, 8, 2), (8, 4, 4)])
def test_epoch_plan(n_files, batch, world):
    plans = [DL.epoch_plan(n_files, batch, rank, world) for rank in range(world)]
    steps = -(-n_files // batch)
    assert all(len(p) == steps for p in plans)
    seen = []
    for s in range(steps):
        size = min(batch, n_files - s * batch)                       # a short last batch, nothing dropped
        cursor = s * batch
        for rank in range(world):
            c, rows = plans[rank][s]
            assert c == cursor                                       # rank slices tile the global batch in rank order
            seen += list(range(c, c + rows))
            cursor += rows
        assert cursor == s * batch + size
    assert seen == list(range(n_files))                              # every permutation slot exactly once per epoch
    assert DL.epoch_seed(3, 0) != DL.epoch_seed(3, 1) != DL.epoch_seed(4, 1)
    with pytest.raises(ValueError):
        DL.epoch_plan(4, 0)
    with pytest.raises(ValueError):
        DL.epoch_plan(4, 2, rank=2, world=2)


def _tree(tmp_path, names, samples, sr=1000, hop=10, n_aunit=1):
    root = str(tmp_path)
    DC.write_tree(root, DC.make_files(names, samples, hop, 3, n_aunit, seed=9), sr)
    return root


def test_refusals_of_the_tree(tmp_path):
    root = _tree(tmp_path / "a", ["1/x", "2/y"], [900, 800])
    assert len(DL.scan_tree(root, 1000, n_spk=2, n_aunit=1)) == 2
    with pytest.raises(ValueError, match="n_spk"):
        DL.scan_tree(root, 1000, n_spk=1, n_aunit=1)
    with pytest.raises(ValueError, match="1000 Hz"):
        DL.scan_tree(root, 2000, n_spk=2, n_aunit=1)
    with pytest.raises(FileNotFoundError, match=r"units\.2"):
        DL.scan_tree(root, 1000, n_spk=2, n_aunit=2)
    for sub in ("f0", "volume"):
        root = _tree(tmp_path / sub, ["1/x"], [900])
        os.remove(os.path.join(root, sub, "1", "x.npy"))
        with pytest.raises(FileNotFoundError, match=sub):
            DL.scan_tree(root, 1000, n_spk=2, n_aunit=1)
    root = _tree(tmp_path / "b", ["spk/x"], [900])
    with pytest.raises(ValueError, match="positive integer"):
        DL.scan_tree(root, 1000, n_spk=2, n_aunit=1)
    root = _tree(tmp_path / "c", ["0/x"], [900])
    with pytest.raises(ValueError, match="n_spk"):
        DL.scan_tree(root, 1000, n_spk=2, n_aunit=1)


def test_refusal_of_a_file_shorter_than_its_longest_crop():
    recs = _records([1000, 900])
    DL.check_lengths(recs, 0.3, 10, 1000)
    recs[1]["f0"] = recs[1]["f0"][:50]                  # 0.9 s: the last start is frame 50, its crop ends at frame 80
    with pytest.raises(ValueError, match="2/f1"):
        DL.check_lengths(recs, 0.3, 10, 1000)
    recs = _records([1000, 900])
    recs[0]["units"][1] = recs[0]["units"][1][:99]      # a whole file of 100 frames
    DL.check_lengths(recs, 0.3, 10, 1000)
    with pytest.raises(ValueError, match="1/f0"):
        DL.check_lengths(recs, 0.3, 10, 1000, whole_audio=True)
    recs = _records([1000, 9])                          # less than one frame
    with pytest.raises(ValueError, match="2/f1"):
        DL.check_lengths(recs, 0.3, 10, 1000, whole_audio=True)
    DL.check_lengths(recs, 0.3, 10, 1000)               # a cropped dataset skips it instead
    with pytest.raises(ValueError, match="units of shape"):
        bad = _records([1000, 900])
        bad[1]["units"][0] = bad[1]["units"][0][:, :2]
        DL.pack_arenas(bad, 0.3)


def test_refusals_of_the_class(tmp_path):
    root = _tree(tmp_path, ["1/x"], [900])
    with pytest.raises(ValueError, match="load_all_data"):
        DL.AudioDataset(root, 0.3, 10, 1000, load_all_data=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DL.AudioDataset(root, 0.3, 10, 1000, device="cpu")
