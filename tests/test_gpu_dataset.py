"""The device-resident dataset: `ddsp_dataset_gather` behind `data_loaders.AudioDataset`.

Yardsticks: tests/golden/dataset_ref.npz - what the reference's own `AudioDataset.__getitem__` returned on the fixture tree
(tests/golden/make_golden_dataset.py) - and, where the tree is made in the test, `dataset_cases.restate`: the reference's
slices written out in torch on the CPU.  A gather copies: every comparison is bit for bit.  Outputs are prefilled with NaN,
so a cell the kernel did not write shows."""
import os

import numpy as np
import pytest
import torch

import data_loaders as DL
import dataset_cases as DC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

KEYS = ("audio", "units", "f0", "volume", "spk_id")


def nan_out(ds, B, Fr, dev):
    C = ds.view.n_unit
    return {"audio": torch.full((B, Fr * ds.hop_size), float("nan"), device=dev),
            "units": torch.full((B, Fr, C), float("nan"), device=dev), "f0": torch.full((B, Fr, 1), float("nan"), device=dev),
            "volume": torch.full((B, Fr), float("nan"), device=dev),
            "spk_id": torch.full((B, 1), -7, device=dev, dtype=torch.int64),
            "draws": torch.full((B, 3), -7, device=dev, dtype=torch.int32)}


def same_bits(got, want, what=""):
    for k in KEYS:
        g = got[k].cpu()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape, want[k].shape)
        assert torch.equal(g, want[k]), (what, k, int((g != want[k]).sum()))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "dataset_ref.npz"))


@pytest.fixture(scope="module")
def fixture_tree(g, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("dataset_fixture"))
    DC.write_tree(root, DC.fixture_files(g), int(g["sr"]))
    return root


def _fixture_ds(g, root, dev, fp16=False, whole_audio=False):
    return DL.AudioDataset(root, float(g["sec"]), int(g["hop"]), int(g["sr"]), whole_audio=whole_audio, n_spk=int(g["n_spk"]),
                           n_aunit=int(g["n_aunit"]), device=dev, fp16=fp16)


def _half(x, fp16):
    return x.half().float() if fp16 else x


@pytest.mark.parametrize("fp16", [False, True])
def test_fixture_parity_cropped(dev, lib_path, g, fixture_tree, fp16):
    ds = _fixture_ds(g, fixture_tree, dev, fp16)
    names = [str(n) for n in g["names"]]
    assert ds.paths == names and len(ds) == len(names)
    triples = [[names.index(str(n)), int(s), int(k)] for n, s, k in zip(g["crop_name"], g["crop_start"], g["crop_unit_idx"])]
    B, Fr = len(triples), DL.crop_frames(float(g["sec"]), int(g["hop"]), int(g["sr"]))
    b = ds.batch(triples, out=nan_out(ds, B, Fr, dev))
    want = {k: torch.from_numpy(g[f"crop_{k}"]) for k in KEYS}
    want["audio"], want["units"] = _half(want["audio"], fp16), _half(want["units"], fp16)
    same_bits(b, want)
    assert b["draws"].cpu().tolist() == triples and b["name"] == [str(n) for n in g["crop_name"]]
    ds.ctx.poll_error()


@pytest.mark.parametrize("fp16", [False, True])
def test_fixture_parity_whole_audio(dev, lib_path, g, fixture_tree, fp16):
    ds = _fixture_ds(g, fixture_tree, dev, fp16, whole_audio=True)
    names = [str(n) for n in g["names"]]
    # three rows of different length in one padded batch: the first reference item of three different files
    rows = {}
    for j, n in enumerate(g["whole_name"]):
        rows.setdefault(names.index(str(n)), j)
    files = sorted(rows)[:3]
    lens = [g[f"whole_f0_{rows[i]}"].shape[0] for i in files]
    assert len(files) == 3 and len(set(lens)) == 3
    Fr = max(lens)
    b = ds.whole_batch(files, unit_idx=[int(g["whole_unit_idx"][rows[i]]) for i in files], out=nan_out(ds, 3, Fr, dev))
    assert b["n_frames"] == lens and b["name"] == [names[i] for i in files]
    hop = int(g["hop"])
    for r, i in enumerate(files):
        j, n = rows[i], lens[r]
        for k, per in (("audio", hop), ("units", 1), ("f0", 1), ("volume", 1)):
            ref = torch.from_numpy(g[f"whole_{k}_{j}"])
            ref = _half(ref, fp16) if k in ("audio", "units") else ref
            got = b[k][r].cpu()
            assert torch.equal(got[:n * per], ref), (k, r)
            assert torch.count_nonzero(got[n * per:]) == 0 and not torch.isnan(got).any(), (k, r)   # exact zeros past the row
        assert int(b["spk_id"][r]) == int(g[f"whole_spk_id_{j}"][0])
    # the compatibility path: one file through the kernel at B = 1, after the reference's skip
    for j, asked in enumerate(g["whole_asked"]):
        item = ds[int(asked)]
        assert item["name"] == str(g["whole_name"][j])
        assert torch.equal(item["f0"].cpu(), torch.from_numpy(g[f"whole_f0_{j}"]))
        assert torch.equal(item["volume"].cpu(), torch.from_numpy(g[f"whole_volume_{j}"]))
        assert torch.equal(item["audio"].cpu(), _half(torch.from_numpy(g[f"whole_audio_{j}"]), fp16))
        assert torch.equal(item["spk_id"].cpu(), torch.from_numpy(g[f"whole_spk_id_{j}"]))
    ds.ctx.poll_error()


# hop 512 with C = 256: 16-byte accesses in both arena types; hop 10 with C = 3: the scalar path; hop 8 with C = 4 in fp16:
# 16-byte audio loads beside 8-byte units loads; hop 4 with C = 4: fp32 vectors beside a scalar fp16 audio copy
@pytest.mark.parametrize("hop,C,fp16", [(512, 256, False), (512, 256, True), (10, 3, False), (10, 3, True), (8, 4, True),
                                        (4, 4, False), (4, 4, True)])
def test_kernel_corners(dev, lib_path, tmp_path, hop, C, fp16):
    sr, sec = hop * 100, 0.1                            # 10 ms frames, crops of 10 frames
    names = ["1/a", "1/b", "2/c", "2/d"]
    samples = [40 * hop + 3, hop, 25 * hop + 1, 33 * hop]
    files = DC.make_files(names, samples, hop, C, 1, seed=hop + C)
    root = DC.write_tree(str(tmp_path), files, sr)
    ds = DL.AudioDataset(root, sec, hop, sr, n_spk=2, n_aunit=1, device=dev, fp16=fp16)
    crop = ds.crop
    assert crop == DL.crop_frames(sec, hop, sr) and 9 <= crop <= 10
    # start 0 in the first file of the arena; a crop that ends on the last usable frame of the LAST file (its audio holds 33
    # frames, its frame series one more); an inner one - and both units copies
    triples = [[0, 0, 0], [3, 33 - crop, 1], [2, 7, 1]]
    b = ds.batch(triples, out=nan_out(ds, 3, crop, dev))
    same_bits(b, DC.restate(files, triples, [crop] * 3, crop, hop, fp16), "crop")
    assert b["draws"].cpu().tolist() == triples
    # whole files: a row 1 frame long beside long ones (first and last file of the arena)
    whole = [1, 0, 3]
    lens = [ds.whole[i] for i in whole]
    assert lens[0] == 1 and lens[1] == 40 and lens[2] in (32, 33)
    b = ds.whole_batch(whole, unit_idx=[1, 0, 1], out=nan_out(ds, 3, max(lens), dev))
    same_bits(b, DC.restate(files, [[1, 0, 1], [0, 0, 0], [3, 0, 1]], lens, max(lens), hop, fp16), "whole")
    assert b["n_frames"] == lens
    ds.ctx.poll_error()


def test_drawn_batches(dev, lib_path, g, fixture_tree):
    ds = _fixture_ds(g, fixture_tree, dev)
    sec, hop, sr = float(g["sec"]), int(g["hop"]), int(g["sr"])
    files = DC.fixture_files(g)
    valid = [i for i, d in enumerate(ds.duration) if not d < sec + 0.1]
    assert 0 < len(valid) < len(ds)
    B = 64
    b = ds.batch(batch_size=B, seed=7, out=nan_out(ds, B, ds.crop, dev))
    draws = b["draws"].cpu().tolist()
    for i, s, k in draws:
        assert i in valid                                                      # a short file never appears
        assert 0 <= s <= DL.max_start_frame(ds.duration[i], sec, hop, sr)      # no start past the reference's largest
        assert 0 <= k <= int(g["n_aunit"])
    assert {i for i, _, _ in draws} == set(valid) and {k for _, _, k in draws} == {0, 1}
    same_bits(b, DC.restate(files, draws, [ds.crop] * B, ds.crop, hop))
    assert ds.batch(batch_size=B, seed=7)["draws"].cpu().tolist() == draws
    assert ds.batch(batch_size=B, seed=8)["draws"].cpu().tolist() != draws
    # a row's draw depends on its place in the permutation, not on the batch it is in
    perm = torch.arange(6, dtype=torch.int32, device=dev)
    whole = ds.batch(batch_size=6, seed=11, perm=perm)["draws"].cpu().tolist()
    assert [i for i, _, _ in whole] == [int(ds.next_valid[i]) for i in range(6)]
    assert ds.batch(batch_size=2, seed=11, perm=perm, cursor=3)["draws"].cpu().tolist() == whole[3:5]
    # the compatibility item of a short file is its successor's
    assert ds[1]["name"] == ds.paths[2] and ds[5]["name"] == ds.paths[0]
    ds.ctx.poll_error()


def test_drawn_starts_cover_exactly_the_possible_ones(dev, lib_path, tmp_path):
    sr, hop, sec = 8000, 80, 0.5
    files = DC.make_files(["1/only"], [5080], hop, 4, 1, seed=3)      # 0.635 s: (0.635 - 0.6) / 0.01 -> starts 0..3
    ds = DL.AudioDataset(DC.write_tree(str(tmp_path), files, sr), sec, hop, sr, n_spk=1, n_aunit=1, device=dev)
    assert DL.max_start_frame(ds.duration[0], sec, hop, sr) == 3
    draws = ds.batch(batch_size=4096, seed=1)["draws"].cpu()
    assert set(draws[:, 0].tolist()) == {0}
    assert int(draws[:, 1].min()) >= 0
    starts = torch.bincount(draws[:, 1].long(), minlength=4)
    print("starts", starts.tolist())
    assert starts.numel() == 4 and int(starts.min()) > 0               # every one of the 4 occurs and nothing else does
    assert set(draws[:, 2].tolist()) == {0, 1}
    ds.ctx.poll_error()


def test_epoch_visits_every_index_once(dev, lib_path, g, fixture_tree):
    ds = _fixture_ds(g, fixture_tree, dev)
    want = sorted(int(ds.next_valid[i]) for i in range(6))
    first = [b["draws"].cpu().tolist() for b in ds.batches(4, seed=5)]
    assert [len(x) for x in first] == [4, 2]                            # a short last batch, nothing dropped
    assert sorted(i for x in first for i, _, _ in x) == want
    second = [b["draws"].cpu().tolist() for b in ds.batches(4, seed=5)]
    assert sorted(i for x in second for i, _, _ in x) == want and second != first     # the next epoch: another order, other crops
    assert [b["draws"].cpu().tolist() for b in ds.batches(4, seed=5, epoch=0)] == first
    # two ranks: their slices of every global batch, put together, are the one-process epoch
    one = [b["draws"].cpu().tolist() for b in ds.batches(4, seed=5, epoch=3)]
    r0 = [b["draws"].cpu().tolist() for b in ds.batches(4, seed=5, rank=0, world=2, epoch=3)]
    r1 = [b["draws"].cpu().tolist() for b in ds.batches(4, seed=5, rank=1, world=2, epoch=3)]
    assert [len(x) for x in r0] == [2, 1] and [len(x) for x in r1] == [2, 1]
    assert [a + b for a, b in zip(r0, r1)] == one
    ds.ctx.poll_error()


def test_bad_triple_sets_the_error_word(dev, lib_path, g, fixture_tree):
    ds = _fixture_ds(g, fixture_tree, dev)
    good = [0, 3, 1]
    ds.ctx.poll_error()
    try:
        for bad in ([0, 101, 0],      # 150 audio frames: a crop of 50 from frame 101 runs off the file
                    [6, 0, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 2]):
            b = ds.batch([good, bad, good], out=nan_out(ds, 3, ds.crop, dev))
            torch.cuda.synchronize()
            with pytest.raises(ValueError, match="triple"):
                ds.batch([good])                                    # the next library call reports it, once
            again = ds.batch([good, good, good])
            torch.cuda.synchronize()
            ds.ctx.poll_error()
            assert b["draws"].cpu().tolist() == [good, bad, good]
            for k in ("audio", "units", "f0", "volume"):
                assert torch.equal(b[k][0], again[k][0]) and torch.equal(b[k][2], again[k][2]), (bad, k)
                assert torch.count_nonzero(b[k][1]) == 0 and not torch.isnan(b[k][1]).any(), (bad, k)   # zeros, nothing read
        ds.batch([good, [0, 10 ** 6, 0]])
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match="triple"):
            ds.ctx.poll_error()
        # argument checks that never reach a launch
        t = torch.tensor([good], dtype=torch.int32, device=dev)
        perm = torch.zeros(4, dtype=torch.int32, device=dev)
        with pytest.raises(ValueError):
            ds.ctx.dataset_gather(ds.view, 1, ds.crop, triples=t, perm=perm, crop_frames=ds.crop)
        with pytest.raises(ValueError):
            ds.ctx.dataset_gather(ds.view, 1, ds.crop, crop_frames=ds.crop)
        with pytest.raises(ValueError):
            ds.ctx.dataset_gather(ds.view, 3, ds.crop, perm=perm, cursor=2, crop_frames=ds.crop, waveform_sec=0.5)
        with pytest.raises(ValueError):
            ds.ctx.dataset_gather(ds.view, 1, ds.crop, triples=t, crop_frames=ds.crop + 1)
        with pytest.raises(ValueError):
            ds.ctx.dataset_gather(ds.view, 1, ds.crop, triples=t.long(), crop_frames=ds.crop)
    finally:
        torch.cuda.synchronize()
        try:
            ds.ctx.poll_error()
        except ValueError:
            pass


def test_end_to_end_train_steps(dev, lib_path, tmp_path):
    import synthetic
    import training
    from ddsp.loss import RSSLoss
    sr, hop, sec = 44100, 512, 0.25
    names = [f"{1 + i % 2}/f{i}" for i in range(6)]
    files = DC.make_files(names, [20000, 17000, 24000, 16000, 22050, 18000], hop, 256, 0, seed=17)
    ds = DL.AudioDataset(DC.write_tree(str(tmp_path), files, sr), sec, hop, sr, n_spk=2, n_aunit=0, device=dev)
    assert (ds.next_valid == np.arange(6)).all() and ds.crop == 21
    model, _ = synthetic.build_model("CombSubFast", seed=3)
    model = model.to(dev).train()
    opt = training.AdamW(model.parameters(), lr=5e-4, weight_decay=0.0)
    crit = RSSLoss(256, 2048, 4, device=dev)
    before = [p.detach().clone() for p in model.parameters()]
    batches = list(ds.batches(4, seed=2))
    assert [b["units"].shape for b in batches] == [(4, 21, 256), (2, 21, 256)]
    losses = [float(training.train_step(model, opt, crit, b, scales=[300, 777, 1531, 2047])) for b in batches]
    assert all(np.isfinite(losses)), losses
    assert any(not torch.equal(p.detach(), q) for p, q in zip(model.parameters(), before))
    assert all(torch.isfinite(p).all() for p in model.parameters())
    whole = next(iter(ds.whole_batches(3 * 47)))
    assert whole["units"].shape[0] == 3 and whole["n_frames"] == sorted(whole["n_frames"], reverse=True)
    loss = float(training.train_step(model, opt, crit, whole, scales=[300, 777, 1531, 2047]))
    assert np.isfinite(loss), loss
    ds.ctx.poll_error()
