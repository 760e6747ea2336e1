"""Generates tests/golden/dataset_ref.npz by running the REFERENCE's `data_loaders.AudioDataset` in this container.

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dataset.py
A tiny tree (tests/dataset_cases.py: 6 PCM16 wavs at 8 kHz, hop 80, 0.3 to 1.5 s, speakers 1/ and 2/, units of 4 channels in
two copies; three files are shorter than waveform_sec + 0.1 = 0.6 s) is written to a temporary directory and read by the
reference's own class, cache on the CPU.  Stand-ins of our own replace what the image lacks: `librosa.load` and
`librosa.get_duration` read the wav with scipy (PCM16 / 32768, samples / rate - what librosa gives for a mono file at its
own rate) and `tqdm` is the identity.  `random.uniform` and `random.randint` are wrapped to log what they return;
`uniform(a, b)` is CPython's own `a + (b - a) * random()` with the `random()` it drew logged beside the result.
The reference lists the files in os.walk order, which is the file system's; the package sorts (`preprocess.list_audio`), so
the reference object's `paths` are sorted here before the first item is asked for, and index i means the same file in both.
Recorded: the tree's arrays (audio as int16); 24 seeded `__getitem__` calls with the asked index, the returned name, the
logged draws and every returned tensor; the same with `whole_audio=True` over all indices.
The reference tree never travels to the GPU box; only the .npz and this script are committed."""
import os
import random
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

from make_golden import REF, save  # noqa: E402
import dataset_cases as DC  # noqa: E402

N_CALLS = 24


def _stand_ins():
    from scipy.io import wavfile

    def load(path, sr=None, mono=True, **kw):
        rate, data = wavfile.read(path)
        assert rate == sr and data.dtype == np.int16 and data.ndim == 1 and not kw
        return data.astype(np.float32) / 32768.0, rate

    def get_duration(filename=None, sr=None, **kw):
        rate, data = wavfile.read(filename)
        return data.shape[0] / rate

    sys.modules["librosa"] = types.ModuleType("librosa")
    sys.modules["librosa"].load = load
    sys.modules["librosa"].get_duration = get_duration
    sys.modules["tqdm"] = types.ModuleType("tqdm")
    sys.modules["tqdm"].tqdm = lambda it, **kw: it


class _LoggedRandom:
    """random.uniform / random.randint that log their results while active."""

    def __enter__(self):
        self.uniform, self.randint = [], []
        self._u, self._r = random.uniform, random.randint

        def uniform(a, b):
            u = random.random()
            ret = a + (b - a) * u          # random.uniform's own body
            self.uniform.append((u, b, ret))
            return ret

        def randint(a, b):
            ret = self._r(a, b)
            self.randint.append(ret)
            return ret

        random.uniform, random.randint = uniform, randint
        return self

    def __exit__(self, *exc):
        random.uniform, random.randint = self._u, self._r


def main():
    _stand_ins()
    sys.path.insert(0, REF)
    import data_loaders as RD   # the reference module
    sys.path.remove(REF)
    assert RD.__file__.startswith(REF)

    files = DC.make_files(DC.NAMES, DC.SAMPLES, DC.HOP, DC.C, DC.N_AUNIT, DC.SEED)
    g = {"names": np.array(DC.NAMES), "sr": DC.SR, "hop": DC.HOP, "sec": DC.SEC, "n_unit": DC.C, "n_aunit": DC.N_AUNIT,
         "n_spk": DC.N_SPK}
    for i, f in enumerate(files):
        g[f"audio_{i}"], g[f"f0_{i}"], g[f"volume_{i}"] = f["audio"], f["f0"], f["volume"]
        for k, u in enumerate(f["units"]):
            g[f"units_{i}_{k}"] = u
    res = DC.HOP / DC.SR
    with tempfile.TemporaryDirectory() as root:
        DC.write_tree(root, files, DC.SR)
        for mode, whole in (("crop", False), ("whole", True)):
            ds = RD.AudioDataset(root, waveform_sec=DC.SEC, hop_size=DC.HOP, sample_rate=DC.SR, load_all_data=True,
                                 whole_audio=whole, n_spk=DC.N_SPK, n_aunit=DC.N_AUNIT, device="cpu", fp16=False)
            ds.paths = sorted(ds.paths)
            assert ds.paths == DC.NAMES
            g["duration"] = np.array([ds.data_buffer[n]["duration"] for n in ds.paths], dtype=np.float64)
            random.seed(DC.SEED + (1 if whole else 0))
            asked = list(range(len(ds))) if whole else [random.randrange(len(ds)) for _ in range(N_CALLS)]
            items, starts = [], []
            with _LoggedRandom() as log:
                for i in asked:
                    items.append(ds[i])
            assert len(log.randint) == len(asked) and len(log.uniform) == (0 if whole else len(asked))
            for j, it in enumerate(items):
                # where the crop starts, as the reference forms it (`data_loaders.py:129`) - and checked against what it returned
                s = 0 if whole else int(log.uniform[j][2] / res)
                f = files[DC.NAMES.index(it["name"])]
                n = it["f0"].shape[0]
                assert np.array_equal(it["f0"][:, 0].numpy(), f["f0"][s:s + n])
                assert np.array_equal(it["audio"].numpy(), (f["audio"].astype(np.float32) / 32768.0)[s * DC.HOP:(s + n) * DC.HOP])
                assert np.array_equal(it["units"].numpy(), f["units"][log.randint[j]][s:s + n])
                starts.append(s)
            g[f"{mode}_asked"] = np.array(asked)
            g[f"{mode}_name"] = np.array([it["name"] for it in items])
            g[f"{mode}_unit_idx"] = np.array(log.randint)
            g[f"{mode}_start"] = np.array(starts)
            if not whole:
                g["crop_u"] = np.array([u for u, _, _ in log.uniform], dtype=np.float64)
                g["crop_hi"] = np.array([b for _, b, _ in log.uniform], dtype=np.float64)
                g["crop_idx_from"] = np.array([r for _, _, r in log.uniform], dtype=np.float64)
                for k in ("audio", "f0", "volume", "units", "spk_id"):
                    g[f"crop_{k}"] = np.stack([it[k].numpy() for it in items])
            else:
                for j, it in enumerate(items):
                    for k in ("audio", "f0", "volume", "units", "spk_id"):
                        g[f"whole_{k}_{j}"] = it[k].numpy()
    save("dataset_ref.npz", **g)


if __name__ == "__main__":
    main()
