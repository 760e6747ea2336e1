"""Generates tests/golden/ref_solver.npz by running the REFERENCE's `solver.test` in this container, on the CPU.

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_solver.py
The five utterances of tests/solver_cases.py (n_spk = 3; 5, 9, 17, 33 and 40 frames; speakers 1, 2, 3, 3, 1; unvoiced
frames with f0 == 0) go through the reference's own validation loop as a list of B = 1 batches.  What the loop is handed:
  model      the reference `CombSub` with the weights of tests/golden/model_CombSub.npz (the product's seeded constructor,
             `seed_weights` there - no second copy is stored), wrapped so that every call is recorded (the mapped f0 and the
             target id of the conversion leg are what the loop passes to its second forward) and the noise of the utterance
             is injected in place of `torch.rand_like`, for both legs;
  loss_func  the reference `RSSLoss` with `torch.randint` replaced for the duration of a call by the pinned scales of
             solver_cases.SCALES; every value is recorded (the loop only returns their mean);
  saver      an object whose `log_audio` does nothing.
Stand-ins of our own for what the image lacks are make_golden.py's (`_placeholders`, `_spectrogram_placeholder`), plus
`logger.saver` / `logger.utils` (the loop imports them and uses neither in `test`; the reference's need TensorBoard).
Recorded: the inputs, `f0_stats`, the mapped f0 and target id per file, the reconstruction the loop scored, the per-file
losses and their mean - data only."""
import contextlib
import io
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as MG  # noqa: E402
import solver_cases as SC  # noqa: E402


class _Args(dict):
    __getattr__ = dict.get


def main():
    import warnings
    warnings.simplefilter("ignore")
    MG._placeholders()
    MG._spectrogram_placeholder()
    import synthetic
    seed = int(np.load(os.path.join(MG.OUT, "model_CombSub.npz"))["seed_weights"])
    prod, cfg = synthetic.build_model("CombSub", seed=seed)
    sd = {k: v.clone() for k, v in prod.state_dict().items()}
    utts = SC.make_utterances()

    MG._fresh_reference("solver", "logger", "logger.saver", "logger.utils")
    logger = types.ModuleType("logger")
    logger.saver = types.ModuleType("logger.saver")
    logger.saver.Saver = None
    logger.utils = types.ModuleType("logger.utils")
    sys.modules.update({"logger": logger, "logger.saver": logger.saver, "logger.utils": logger.utils})
    import ddsp.loss as RL
    import ddsp.vocoder as V
    import solver as RS
    assert all(m.__file__.startswith(MG.REF) for m in (RL, V, RS))
    sys.path.remove(MG.REF)

    ref = V.CombSub(SC.SR, SC.HOP, cfg["n_mag_allpass"], cfg["n_mag_harmonic"], cfg["n_mag_noise"], SC.N_UNIT, cfg["n_spk"])
    ref.load_state_dict(sd, strict=True)

    class Model:
        calls, signals = [], []

        def eval(self):
            ref.eval()

        def __call__(self, units, f0, volume, spk_id):
            noise = torch.from_numpy(utts[len(self.calls) // 2]["noise"])
            self.calls.append((f0.clone(), spk_id.clone()))
            with MG._InjectNoise(noise):
                out = ref(units, f0, volume, spk_id)
            self.signals.append(out[0].detach().clone())
            return out

    crit = RL.RSSLoss(SC.FFT_MIN, SC.FFT_MAX, SC.N_SCALE, device="cpu")
    values = []

    def loss_func(x_pred, x_true):
        orig = torch.randint
        torch.randint = lambda lo, hi, size: torch.tensor(SC.SCALES)
        try:
            values.append(crit(x_pred, x_true))
        finally:
            torch.randint = orig
        return values[-1]

    loader = [{"name": [u["name"]], "units": torch.from_numpy(u["units"])[None], "f0": torch.from_numpy(u["f0"])[None, :, None],
               "volume": torch.from_numpy(u["volume"])[None], "spk_id": torch.tensor([[u["spk_id"]]], dtype=torch.int64),
               "audio": torch.from_numpy(u["audio"][:len(u["noise"])])[None]} for u in utts]
    model = Model()
    with tempfile.TemporaryDirectory() as root:
        np.save(os.path.join(root, "f0_stats"), SC.F0_STATS)
        args = _Args(device="cpu", data=_Args(train_path=root, sampling_rate=SC.SR), model=_Args(n_spk=SC.N_SPK))
        with contextlib.redirect_stdout(io.StringIO()):
            mean = RS.test(args, model, loss_func, loader, types.SimpleNamespace(log_audio=lambda d: None))
    assert len(model.calls) == 2 * len(utts) and len(values) == len(utts)

    g = {"names": np.array(SC.NAMES), "spk": np.array(SC.SPK, dtype=np.int64), "frames": np.array(SC.FRAMES),
         "scales": np.array(SC.SCALES), "n_spk": SC.N_SPK, "seed_weights": seed,
         "f0_stats_keys": np.array(list(SC.F0_STATS)), "f0_stats_values": np.array(list(SC.F0_STATS.values()), dtype=np.float64),
         "losses": np.array([float(v) for v in values], dtype=np.float64), "mean": float(mean)}
    for i, u in enumerate(utts):
        for k in ("units", "f0", "volume", "audio", "noise"):
            g[f"{k}_{i}"] = u[k]
        rec_f0, rec_spk = model.calls[2 * i]
        assert np.array_equal(rec_f0[0, :, 0].numpy(), u["f0"]) and int(rec_spk) == u["spk_id"]
        vc_f0, vc_spk = model.calls[2 * i + 1]
        g[f"f0_vc_{i}"] = vc_f0[0, :, 0].numpy()
        g[f"pred_{i}"] = model.signals[2 * i][0].numpy()          # the reconstruction the loop scored
        g.setdefault("tgt", []).append(int(vc_spk))
        assert np.all(np.isfinite(g[f"f0_vc_{i}"])) and np.all(g[f"f0_vc_{i}"][u["f0"] == 0] == 0)
    g["tgt"] = np.array(g["tgt"], dtype=np.int64)
    assert abs(g["losses"].mean() - g["mean"]) < 1e-12 and np.all(np.isfinite(g["losses"]))
    MG.save("ref_solver.npz", **g)
    print("targets", g["tgt"], "losses", g["losses"], "mean", g["mean"])


if __name__ == "__main__":
    main()
