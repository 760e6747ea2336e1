"""What a validation pass costs: `solver.validate` (ragged groups, one read-back) against the reference-shaped per-file loop
restated here on the same build - per file two B = 1 forwards, the f0 map in torch with the speaker id read on the host, one
loss call and one `.item()` (`solver.py:29-77`).  Run on the GPU box, one session:
    python tools/validate_time.py [--out profiles/validate_time.json]
32 utterances of 2 to 10 s at 44.1 kHz / hop 512, 4 speakers, CombSub, scales pinned.  Per leg: wall time of a pass (the clock
stops after the pass's last synchronisation; median of 5 passes after 2 of warm-up, the legs alternating) and the mean
loss, which the two legs must agree on."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ddsp-svc-official_amd"))
import data_loaders as DL  # noqa: E402
import solver  # noqa: E402
import synthetic  # noqa: E402
from ddsp.loss import RSSLoss  # noqa: E402
from logger.utils import DotDict  # noqa: E402

SR, HOP, C, N_SPK = 44100, 512, 256, 4
SCALES = [300, 777, 1200, 2000]
STATS = {"1": 5.2, "2": 5.6, "3": 4.9, "4": 5.4}


def make_records(n_files, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    recs = []
    for i in range(n_files):
        fr = int(rng.integers(2 * SR // HOP, 10 * SR // HOP))
        inp = synthetic.make_inputs(seed + 1 + i, 1, fr, with_noise=False)
        recs.append({"name": f"{1 + i % N_SPK}/f{i:04d}", "audio": 0.1 * rng.standard_normal(fr * HOP + 64, dtype=np.float32),
                     "duration": (fr * HOP + 64) / SR, "spk_id": 1 + i % N_SPK, "f0": inp["f0"][0, :, 0].numpy(),
                     "volume": inp["volume"][0].numpy(), "units": [inp["units"][0].numpy()]})
    return recs


def per_file_loop(args, model, crit, ds, lfo_stats):
    """The reference's loop with this build's model and loss, a file at a time."""
    total = 0.0
    with torch.no_grad():
        for i in range(len(ds)):
            b = ds.whole_batch([i])
            pred = model(b["units"], b["f0"], b["volume"], b["spk_id"])[0]
            src = int(b["spk_id"].item())                                  # the speaker ids decide the map on the host
            tgt = solver.target_speaker(src, args.model.n_spk)
            ratio = torch.tensor(lfo_stats[str(tgt)] / lfo_stats[str(src)], dtype=torch.float32).to(ds.device)
            model(b["units"], torch.exp(ratio * torch.log(b["f0"])), b["volume"], torch.full_like(b["spk_id"], tgt))
            crit.set_scales(SCALES)
            total += crit(pred, b["audio"]).item()
    return total / len(ds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate_time.json"))
    cmd = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("validate_time needs a HIP device: a CPU run gives no time")
    dev = torch.device("cuda:0")
    ds = DL.AudioDataset(None, 2.0, HOP, SR, whole_audio=True, n_spk=N_SPK, device=dev, records=make_records(cmd.files))
    torch.manual_seed(1)
    from ddsp.vocoder import CombSub
    model = CombSub(SR, HOP, 256, 512, 256, C, N_SPK).to(dev).eval()
    crit = RSSLoss(256, 2048, 4, device=dev)
    res = {"device": torch.cuda.get_device_name(0), "files": cmd.files, "audio_s": sum(ds.whole) * HOP / SR, "scales": SCALES,
           "groups": len(list(DL.group_segments(ds.whole, solver.VAL_BATCH_FRAMES)))}
    with tempfile.TemporaryDirectory() as root:
        np.save(os.path.join(root, "f0_stats"), STATS)
        args = DotDict({"data": {"train_path": root, "sampling_rate": SR}, "model": {"n_spk": N_SPK}})
        legs = {"validate": lambda: solver.validate(args, model, crit, ds, scales=SCALES),
                "per_file_loop": lambda: per_file_loop(args, model, crit, ds, STATS)}
        times, loss = {k: [] for k in legs}, {}
        for rep in range(7):
            for name, leg in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loss[name] = leg()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[name].append(time.perf_counter() - t0)
    for name in legs:
        res[name] = {"ms_per_pass_median": 1e3 * float(np.median(times[name])), "ms_per_pass_all": [1e3 * t for t in times[name]],
                     "mean_loss": loss[name]}
    res["ratio_loop_over_validate"] = res["per_file_loop"]["ms_per_pass_median"] / res["validate"]["ms_per_pass_median"]
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(cmd.out)), exist_ok=True)
    with open(cmd.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
