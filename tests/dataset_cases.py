"""Shared by tests/golden/make_golden_dataset.py, tests/test_dataset_host.py and tests/test_gpu_dataset.py: the tiny dataset
tree of the fixture, a writer of the tree `preprocess.py` produces, and a torch-slicing restatement of a batch."""
import os

import numpy as np
import torch

# the fixture's settings (tests/golden/dataset_ref.npz)
SR, HOP, SEC, C, N_AUNIT, N_SPK = 8000, 80, 0.5, 4, 1, 2
NAMES = ["1/u0", "1/u1", "1/u2", "2/u3", "2/u4", "2/u5"]
# samples: 1.5 s; 0.3 s (skipped); 0.62 s (3 possible starts); 0.55 s (skipped); 1.2 s and 11 samples; 0.375 s (skipped, the
# last file: its skip wraps round to file 0)
SAMPLES = [12000, 2400, 4960, 4400, 9611, 3000]
SEED = 20240611


def make_files(names, samples, hop, n_unit, n_aunit, seed, extra_frames=1):
    """Seeded file records as `preprocess.py` would leave them: PCM16 audio, and len // hop + extra_frames frames of f0,
    volume and (n_aunit + 1) units copies."""
    rng = np.random.Generator(np.random.PCG64(seed))
    files = []
    for name, n in zip(names, samples):
        fr = n // hop + extra_frames
        files.append({
            "name": name,
            "audio": rng.integers(-20000, 20000, size=n).astype(np.int16),
            "f0": rng.uniform(80.0, 600.0, size=fr).astype(np.float32),
            "volume": rng.uniform(0.0, 0.3, size=fr).astype(np.float32),
            "units": [rng.standard_normal((fr, n_unit)).astype(np.float32) for _ in range(n_aunit + 1)],
        })
    return files


def write_tree(root, files, sr):
    """<root>/audio/<name>.wav (PCM16), f0/<name>.npy, volume/<name>.npy, units/<name>.<k>.npy."""
    from scipy.io import wavfile
    for f in files:
        for sub in ("audio", "f0", "volume", "units"):
            os.makedirs(os.path.dirname(os.path.join(root, sub, f["name"])), exist_ok=True)
        wavfile.write(os.path.join(root, "audio", f["name"] + ".wav"), sr, f["audio"])
        np.save(os.path.join(root, "f0", f["name"] + ".npy"), f["f0"])
        np.save(os.path.join(root, "volume", f["name"] + ".npy"), f["volume"])
        for k, u in enumerate(f["units"]):
            np.save(os.path.join(root, "units", f["name"] + f".{k}.npy"), u)
    return root


def fixture_files(g):
    """The file records stored in the loaded fixture `g`."""
    names = [str(n) for n in g["names"]]
    return [{"name": n, "audio": g[f"audio_{i}"], "f0": g[f"f0_{i}"], "volume": g[f"volume_{i}"],
             "units": [g[f"units_{i}_{k}"] for k in range(int(g["n_aunit"]) + 1)]} for i, n in enumerate(names)]


def restate(files, triples, lens, Fr_out, hop, fp16=False):
    """What a batch must hold, by slicing as the reference does (`data_loaders.py:140-144`): row b is `lens[b]` frames of
    file triples[b][0] from frame triples[b][1] on, units copy triples[b][2], zeros up to Fr_out.  PCM16 audio is scaled
    as `preprocess.load_wav` does; with `fp16` audio and units go through half precision first."""
    B = len(triples)
    n_unit = files[0]["units"][0].shape[1]
    out = {"audio": torch.zeros(B, Fr_out * hop), "units": torch.zeros(B, Fr_out, n_unit), "f0": torch.zeros(B, Fr_out, 1),
           "volume": torch.zeros(B, Fr_out), "spk_id": torch.zeros(B, 1, dtype=torch.int64)}
    for b, ((i, s, k), n) in enumerate(zip(triples, lens)):
        f = files[i]
        audio = torch.from_numpy(f["audio"].astype(np.float32) / 32768.0)
        units = torch.from_numpy(f["units"][k])
        if fp16:
            audio, units = audio.half().float(), units.half().float()
        a = audio[s * hop:(s + n) * hop]
        u = units[s:s + n]
        assert a.shape[0] == n * hop and u.shape[0] == n, "the restatement's own slice ran off the file"
        out["audio"][b, :n * hop] = a
        out["units"][b, :n] = u
        out["f0"][b, :n, 0] = torch.from_numpy(f["f0"])[s:s + n]
        out["volume"][b, :n] = torch.from_numpy(f["volume"])[s:s + n]
        out["spk_id"][b, 0] = int(os.path.dirname(f["name"]))
    return out
