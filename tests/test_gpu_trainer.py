"""The training loop on the device (`solver`, `logger`, `train`): the conversion leg's f0 map, ragged validation against the
reference's own `solver.test` run (tests/golden/ref_solver.npz, made by tests/golden/make_golden_solver.py) and against the
reference-shaped per-file loop written here, checkpoints that resume bit for bit, and a short `solver.train` run.

Tolerance of a validation loss (model forward, then the loss) against the reference's run: 2e-4 relative, the one
tests/test_gpu_training.py applies to `train_step`'s loss against the reference's training run - the same two stages."""
import os
import types

import numpy as np
import pytest
import torch

import solver_cases as SC
import synthetic

pytestmark = pytest.mark.gpu
TOL = 2e-4
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def case(dev, lib_path, tmp_path_factory):
    from data_loaders import AudioDataset
    from logger.utils import DotDict
    z = SC.load()
    root = tmp_path_factory.mktemp("solver")
    np.save(os.path.join(root, "f0_stats"), SC.f0_stats(z))
    dataset = AudioDataset(None, waveform_sec=0.5, hop_size=SC.HOP, sample_rate=SC.SR, whole_audio=True, n_spk=SC.N_SPK,
                           device=dev, records=SC.records(z))
    assert dataset.whole == [int(k) for k in z["frames"]]
    model, cfg = synthetic.build_model("CombSub", seed=int(z["seed_weights"]), device=dev)
    args = DotDict({"device": "cuda", "env": {"expdir": str(root / "exp"), "gpu_id": 0},
                    "data": {"train_path": str(root), "sampling_rate": SC.SR, "block_size": SC.HOP, "encoder_out_channels": SC.N_UNIT},
                    "model": {"type": "CombSub", "n_spk": SC.N_SPK, "n_mag_allpass": 256, "n_mag_harmonic": 512, "n_mag_noise": 256},
                    "loss": {"fft_min": SC.FFT_MIN, "fft_max": SC.FFT_MAX, "n_scale": SC.N_SCALE, "val_scales": [int(s) for s in z["scales"]]},
                    "train": {"epochs": 30, "interval_log": 10, "interval_val": 15, "val_batch_frames": 40}})
    noise = {str(name): torch.from_numpy(z[f"noise_{i}"]) for i, name in enumerate(z["names"])}
    return types.SimpleNamespace(z=z, dataset=dataset, model=model, args=args, noise=noise, root=root,
                                 scales=[int(s) for s in z["scales"]])


def _crit(dev):
    from ddsp.loss import RSSLoss
    return RSSLoss(SC.FFT_MIN, SC.FFT_MAX, SC.N_SCALE, device=dev)


def test_vc_f0_map_against_the_reference_run(ctx, dev, case):
    """fp32 on both sides, the reference's order of operations: y = lfo_t * ln(f0) / lfo_s, out = exp(y).  The logarithm (at
    most 1 ulp on the device), the product and the quotient (correctly rounded: 1/2 ulp each) leave y with a relative error
    of at most 2 eps, which exp turns into a relative error of |y| * 2 eps of the result, and exp adds 1 ulp of its own:
    (2 |y| + 1) eps per side, twice that between two sides that each round - with |y| the largest ln of a mapped f0."""
    z = case.z
    n, Fr, B = [int(k) for k in z["frames"]], int(max(z["frames"])), len(z["frames"])
    f0, want = torch.zeros(B, Fr, 1), np.zeros((B, Fr), dtype=np.float32)
    for i, k in enumerate(n):
        f0[i, :k, 0] = torch.from_numpy(z[f"f0_{i}"])
        want[i, :k] = z[f"f0_vc_{i}"]
    f0[:, :, 0] += torch.where(torch.arange(Fr)[None] >= torch.tensor(n)[:, None], 440.0, 0.0)     # a decoy past every row's end
    import solver
    lfo = torch.from_numpy(solver.lfo_table(SC.f0_stats(z), SC.N_SPK)).to(dev)
    spk = torch.from_numpy(z["spk"]).reshape(B, 1).to(dev)
    got, tgt = ctx.vc_f0_map(f0.to(dev), spk, lfo, ctx.ragged_counts(n))
    assert got.shape == (B, Fr, 1) and tgt.shape == (B, 1) and tgt.dtype == torch.int64
    assert tgt.reshape(-1).tolist() == [int(t) for t in z["tgt"]]
    got = got.cpu().numpy()[:, :, 0]
    assert np.array_equal(got == 0, want == 0)                          # unvoiced frames and the padding: exact zeros, no NaN
    rtol = 2 * (2 * float(np.log(want.max())) + 1) * EPS
    err = np.abs(got - want)[want > 0] / want[want > 0]
    print("vc_f0_map: largest relative error", err.max(), "bound", rtol)
    assert err.max() <= rtol
    full, _ = ctx.vc_f0_map(f0.to(dev), spk, lfo)                        # without counts every frame is mapped
    assert bool((full[:, :, 0].cpu() > 0).sum() == (f0[:, :, 0] > 0).sum())
    with pytest.raises(ValueError):
        ctx.vc_f0_map(f0.to(dev), spk.int(), lfo)


def _reference_shaped_loop(case, crit):
    """`solver.py:29-77` with the existing pieces: per file one B = 1 forward of the model and one loss call with the same
    scales and noise (the conversion forward does not enter the loss)."""
    z, dev = case.z, case.dataset.device
    total = []
    with torch.no_grad():
        for i, k in enumerate(z["frames"]):
            sig = case.model(torch.from_numpy(z[f"units_{i}"])[None].to(dev), torch.from_numpy(z[f"f0_{i}"])[None, :, None].to(dev),
                             torch.from_numpy(z[f"volume_{i}"])[None].to(dev), torch.tensor([[int(z["spk"][i])]]).to(dev),
                             noise=torch.from_numpy(z[f"noise_{i}"])[None].to(dev))[0]
            crit.set_scales(case.scales)
            total.append(crit(sig, torch.from_numpy(z[f"audio_{i}"][:int(k) * SC.HOP])[None].to(dev)).item())
    return np.array(total)


def test_validate_against_the_reference_run_and_the_per_file_loop(dev, case):
    import solver
    crit = _crit(dev)
    want = case.z["losses"]
    loop = _reference_shaped_loop(case, crit)
    passes = {}
    for tag, batch_frames in (("one group", 10 ** 6), ("groups of at most 2 rows", 40)):
        groups = [len(b["n_frames"]) for b in case.dataset.whole_batches(batch_frames)]
        assert (groups == [5]) if batch_frames > 40 else (max(groups) == 2 and len(groups) == 4)
        d = {}
        mean = solver.validate(case.args, case.model, crit, case.dataset, batch_frames=batch_frames, scales=case.scales,
                               noise=case.noise, details=d)
        got = np.array([d["losses"][d["names"].index(str(name))] for name in case.z["names"]])
        print(tag, "validate", got, "fixture", want, "loop", loop)
        assert np.all(np.abs(got - want) < TOL * want) and abs(mean - float(case.z["mean"])) < TOL * float(case.z["mean"])
        assert np.all(np.abs(got - loop) < TOL * loop) and abs(mean - loop.mean()) < TOL * loop.mean()
        assert abs(mean - got.mean()) < 1e-12 and d["rtf"] > 0
        passes[tag] = got
    a, b = passes.values()
    assert np.all(np.abs(a - b) < TOL * b)
    assert not case.model.training


def test_validate_reads_the_host_once(dev, case, monkeypatch):
    """Counted, not timed: every synchronising read-back of a device tensor in the pass (`.cpu()`, `.item()`, `.tolist()`,
    `.numpy()`, `float()` / `int()` / `bool()`) goes through the wrappers below; the pass of four groups makes exactly one, the
    `.cpu()` of the concatenated losses.  `solver.test` through a saver takes the same path."""
    import solver
    from logger.saver import Saver
    crit = _crit(dev)
    solver.validate(case.args, case.model, crit, case.dataset, batch_frames=40)         # (contexts, tables: built before counting)
    seen = []
    for name in ("cpu", "item", "tolist", "numpy", "__float__", "__int__", "__bool__"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                seen.append(_name)
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    solver.validate(case.args, case.model, crit, case.dataset, batch_frames=40, scales=case.scales)
    assert seen == ["cpu"], seen
    seen.clear()
    saver = Saver(case.args, initial_global_step=0)
    solver.test(case.args, case.model, crit, types.SimpleNamespace(dataset=case.dataset), saver)
    assert seen == ["cpu"], seen
    assert crit.last_scales == case.scales                                # args.loss.val_scales pinned the draw


def _batch(dev, seed, B, Fr, target_seed):
    batch = {k: v.to(dev) for k, v in synthetic.make_inputs(seed, B, Fr, n_spk=SC.N_SPK).items()}
    with torch.no_grad():                                                 # a reachable target: the output of other weights
        other, _ = synthetic.build_model("CombSub", seed=target_seed, device=dev)
        batch["audio"] = other(batch["units"], batch["f0"], batch["volume"], batch["spk_id"], noise=batch["noise"])[0]
    return batch


def test_checkpoint_resumes_bit_for_bit(dev, case, tmp_path):
    import training
    from logger import utils
    from logger.saver import Saver
    from logger.utils import DotDict
    batch = _batch(dev, 4100, 2, 24, 5)
    args = DotDict(dict(case.args, env={"expdir": str(tmp_path), "gpu_id": 0}))

    def run(resume):
        model, _ = synthetic.build_model("CombSub", seed=21, device=dev)
        model.train()
        opt = training.AdamW(model.parameters(), lr=3e-4, weight_decay=0.01)
        crit = _crit(dev)
        for s in range(2):
            torch.manual_seed(100 + s)
            training.train_step(model, opt, crit, batch, scales=case.scales)
        if resume:
            saver = Saver(args, initial_global_step=2)
            saver.save_model(model, opt, postfix="2")
            fresh, _ = synthetic.build_model("CombSub", seed=22, device=dev)
            fresh_opt = training.AdamW(fresh.parameters())
            step, fresh, fresh_opt = utils.load_model(str(tmp_path), fresh.train(), fresh_opt, device="cuda")
            assert step == 2
            for (n, p), q in zip(model.named_parameters(), fresh.parameters()):
                assert torch.equal(p, q), n
                a, b = opt.state[p], fresh_opt.state[q]
                assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"]), n
                assert float(a["step"]) == float(b["step"]) == 2.0 and not b["step"].is_cuda
            assert fresh_opt.param_groups[0]["lr"] == 3e-4 and fresh_opt.param_groups[0]["weight_decay"] == 0.01
            model, opt = fresh, fresh_opt
        torch.manual_seed(102)
        return training.train_step(model, opt, crit, batch, scales=case.scales).item()

    first, second, resumed = run(False), run(False), run(True)
    print("uninterrupted", first, second, "resumed", resumed)
    if first == second:
        assert resumed == first
    else:
        assert abs(resumed - first) <= 4 * abs(first - second)


def test_train_runs_validates_and_writes_checkpoints(dev, case, tmp_path):
    import solver
    import training
    from ddsp.vocoder import CombSub, load_model
    from logger.utils import DotDict
    args = DotDict(dict(case.args, env={"expdir": str(tmp_path / "exp"), "gpu_id": 0}))
    torch.manual_seed(31)
    model = CombSub(SC.SR, SC.HOP, 256, 512, 256, SC.N_UNIT, SC.N_SPK).to(dev)
    batch = _batch(dev, 4200, 4, 43, 6)                                   # B = 4, 0.5 s crops (43 frames)
    opt = training.AdamW(model.parameters(), lr=3e-4, weight_decay=0.0)
    crit = _crit(dev)

    def loss_now():
        model.eval()
        with torch.no_grad():
            sig = model(batch["units"], batch["f0"], batch["volume"], batch["spk_id"], noise=batch["noise"])[0]
            crit.set_scales(case.scales)
            return crit(sig, batch["audio"]).item()

    before = loss_now()
    solver.train(args, 0, model, opt, crit, [batch], types.SimpleNamespace(dataset=case.dataset), max_steps=30, scales=case.scales)
    after = loss_now()
    print("loss before", before, "after 30 steps", after)
    assert np.isfinite(after) and after < before
    exp = tmp_path / "exp"
    for f in ("model_best.pt", "model_15.pt", "model_30.pt", "config.yaml", "log_info.txt"):
        assert (exp / f).exists(), f
    assert torch.load(exp / "model_30.pt", weights_only=True)["global_step"] == 30
    loaded, largs = load_model(str(exp / "model_best.pt"), device=dev)
    assert largs.model.type == "CombSub" and largs.model.n_spk == SC.N_SPK
    with torch.no_grad():
        audio = loaded(batch["units"], batch["f0"], batch["volume"], batch["spk_id"])[0]
    assert audio.shape == (4, 43 * SC.HOP) and bool(torch.isfinite(audio).all()) and float(audio.abs().max()) > 0
