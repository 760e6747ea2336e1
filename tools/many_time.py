"""Timing of the conversion of a folder of short utterances: a loop of `infer_offline.convert_device` over N files against ONE
`infer_offline.convert_many_device` of the same N files, in one session, the two legs alternating.

    python tools/many_time.py [--files 8 64] [--rounds R] [--warmup W] [--out profiles/many_time.json]

The files: N synthetic utterances of 2 to 6 s at 44.1 kHz (a gliding harmonic tone over a noise floor), each cut into slices of
0.8 to 1.6 s with gaps of 0.1 s between them (given `slices`, the same for both legs).  CombSub with seeded weights, the
HuBERT-Soft encoder and the shipped NSF-HiFiGAN shape with the deterministic fills of the tests, `F0_Extractor('ac')`.
Both legs use the same budgets (`batch_frames`, `units_batch_samples`, `enhancer_batch_samples`); the loop's groups hold the
slices of one file, the many-file call's those of all files.  Each leg is a wall-clock time around work that ends with every
file's result on the device (one synchronisation at the end); the median over the rounds is reported, with and without the
enhancer.  Two further, untimed passes of each leg count what it puts on the device: under `torch.profiler` every device
activity of the process - the library's kernels, ATen's own (the `stack_rows` copies, `.clone()`, `index_select`, slicing) and the
memory copies - which is the launch count per file (`device_ops_per_file_*`; null where the profiler records no device
activity); and under the library's profiler its brackets (`Context.profile_begin`: one kernel or a tight group each, ATen's
launches not among them - not a launch count).
Both legs are given the same `slices`, so the slicer call and its read-back, which the loop pays per file and `analyse_many`
once, are not in the measurement."""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ddsp-svc-official_amd"), os.path.join(ROOT, "tests")]

import glue_cases as GC  # noqa: E402
import hubert_cases as HC  # noqa: E402
import hipddsp  # noqa: E402
import infer_offline  # noqa: E402
import synthetic  # noqa: E402

SR, HOP = 44100, 512
NSF = dict(GC.NSF_CONFIG, upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4], upsample_initial_channel=512,
           num_mels=128, hop_size=512, n_fft=2048, win_size=2048)
BUDGETS = dict(batch_frames=4096, units_batch_samples=2000000, enhancer_batch_samples=1500000)


def utterances(n, seed=23):
    """-> ([audio (T,) fp32 numpy], [[(start_sample, end_sample)]]): n files of 2 to 6 s and their slices."""
    rng = np.random.Generator(np.random.PCG64(seed))
    audios, slices = [], []
    for _ in range(n):
        T = int(rng.uniform(2.0, 6.0) * SR)
        t = np.arange(T) / SR
        f = rng.uniform(100.0, 260.0) * np.exp(np.log(1.5) * t / t[-1])
        ph = 2 * np.pi * np.cumsum(f) / SR
        audios.append((0.3 * np.sin(ph) + 0.12 * np.sin(2 * ph + 0.3) + 0.01 * rng.standard_normal(T)).astype(np.float32))
        cuts, at = [], 0
        while T - at > int(0.5 * SR):
            end = min(T, at + int(rng.uniform(0.8, 1.6) * SR))
            cuts.append((at, end))
            at = end + int(0.1 * SR)
        slices.append(cuts)
    return audios, slices


def front(dev, tmp):
    from ddsp.hubert import HubertSoft
    from ddsp.vocoder import F0_Extractor, Units_Encoder
    from enhancer import Enhancer
    path = os.path.join(tmp, "hubert-soft.pt")
    torch.save(HC.fill({k: tuple(v.shape) for k, v in HubertSoft().state_dict().items()}), path)
    with open(os.path.join(tmp, "config.json"), "w") as fh:
        json.dump(NSF, fh)
    torch.save({"generator": GC.nsf_state_dict(NSF, seed=91)}, os.path.join(tmp, "model"))
    with contextlib.redirect_stdout(sys.stderr):
        return (Units_Encoder("hubertsoft", path, device=dev), F0_Extractor("ac", SR, HOP, 65.0, 800.0, device=dev),
                Enhancer("nsf-hifigan", os.path.join(tmp, "model"), device=dev))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def launches(ctx, fn):
    ctx.profile_begin()
    fn()
    torch.cuda.synchronize()
    return int(sum(v["launches"] for v in ctx.profile_end().values()))


def device_ops(fn):
    """Device activities (kernels and memory copies) of one call of fn, from torch.profiler; None where it records none."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)
    return n or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = hipddsp.context_for(dev)
    from ddsp.vocoder import DotDict
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    model, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    encoder, extractor, enhancer = front(dev, tempfile.mkdtemp())
    spk = torch.full((1, 1), 2, dtype=torch.int64, device=dev)
    rows = []
    for n in a.files:
        audios, slices = utterances(n)
        on_dev = [torch.from_numpy(x).to(dev) for x in audios]
        for enh in (None, enhancer):
            kw = dict(BUDGETS, enhancer=enh, noise_seed=5)
            if enh is None:
                kw.pop("enhancer_batch_samples")

            def loop():
                return [infer_offline.convert_device(model, args, x, SR, s, encoder, extractor, spk, **kw)[0]
                        for x, s in zip(on_dev, slices)]

            def many():
                return infer_offline.convert_many_device(model, args, on_dev, SR, encoder, extractor, 2, slices=slices, **kw)

            for _ in range(a.warmup):
                loop(), many()
            ms = {"loop": [], "many": []}
            for _ in range(a.rounds):                     # the legs alternate: drift of the clocks hits both alike
                ms["loop"].append(wall(loop))
                ms["many"].append(wall(many))
            per_file = loop()
            out, spans, _ = many()
            assert [int(x.numel()) for x in per_file] == [t for _, t in spans], "the two legs give files of different length"
            n_loop, n_many = launches(ctx, loop), launches(ctx, many)
            ops_loop, ops_many = device_ops(loop), device_ops(many)
            ctx.poll_error()
            med = {k: float(np.median(v)) for k, v in ms.items()}
            row = {"files": n, "slices": sum(len(s) for s in slices), "seconds_of_audio": sum(len(x) for x in audios) / SR,
                   "enhancer": enh is not None, "loop_wall_ms": med["loop"], "many_wall_ms": med["many"],
                   "loop_wall_ms_min_max": [min(ms["loop"]), max(ms["loop"])], "many_wall_ms_min_max": [min(ms["many"]), max(ms["many"])],
                   "loop_over_many": med["loop"] / med["many"], "loop_ms_per_file": med["loop"] / n, "many_ms_per_file": med["many"] / n,
                   "device_ops_per_file_loop": ops_loop and ops_loop / n, "device_ops_per_file_many": ops_many and ops_many / n,
                   "library_brackets_per_file_loop": n_loop / n, "library_brackets_per_file_many": n_many / n,
                   "rounds": a.rounds, "warmup": a.warmup, **{k: v for k, v in BUDGETS.items() if k in kw}}
            print(json.dumps(row), flush=True)
            rows.append(row)
    result = {"device": torch.cuda.get_device_name(0), "model": "CombSub", "f0": "ac", "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
