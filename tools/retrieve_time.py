"""What unit retrieval costs: one `Context.units_retrieve_` call against the same search written in torch (`cdist`, `topk`,
gather, weights, blend), and the 16-stream 0.2 s block of tools/rt_bank_time.py with and without an index on every slot.

The call: rows x 75 frames, rows in (1, 16), C in (256, 768), N in (10 000, 200 000), k = 8, ratio 0.5.  Both forms run in ONE
process and ALTERNATE call by call (HIP events around each; a warm-up first), so clocks and other tenants move both alike; the
median and the fastest of `--repeats` calls are written, with the time the index's bytes alone take at `--hbm-tbs` TB/s (the
floor of a search that reads the index once) and the ratio of the kernel's median to it.  The torch form allocates an (rows * 75,
N) matrix per call, which is the point of the comparison.

The bank: S = 16 streams, 0.2 s blocks at 48 kHz (config5 of rt_bank_time.py), random-weight CREPE and HuBERT-Soft; two banks in
one process, one built with `indices=` and an index of `--bank-entries` entries on every slot, one without, pushed alternately.

    python tools/retrieve_time.py [--out profiles/retrieve_time.json] [--repeats 20] [--skip-bank]"""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ddsp-svc-official_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES, K, RATIO = 75, 8, 0.5


def torch_retrieve(x, vec, k, ratio):
    """The rule with torch operators: the yardstick for time, not for bits."""
    import torch
    rows, Fr, C = x.shape
    q = x.reshape(-1, C)
    d = torch.cdist(q, vec) ** 2
    s, ids = torch.topk(d, k, dim=1, largest=False)
    w = 1.0 / torch.clamp(s, min=1e-12) ** 2
    w = w / w.sum(1, keepdim=True)
    y = (w[:, :, None] * vec[ids]).sum(1)
    return (q + ratio * (y - q)).reshape(rows, Fr, C)


def time_calls(a, repeats, warmup=3):
    """Alternate the two forms; -> {name: [ms]}."""
    import torch
    out = {name: [] for name in a}
    for i in range(warmup + repeats):
        for name, fn in a.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            if i >= warmup:
                out[name].append(start.elapsed_time(stop))
    return out


def calls(repeats, hbm_tbs):
    import numpy as np
    import torch

    import hipddsp
    from infer_offline import UnitIndex, UnitIndexBank
    dev = torch.device("cuda:0")
    ctx = hipddsp.context_for(dev)
    rows_out = []
    for C in (256, 768):
        for N in (10_000, 200_000):
            g = torch.Generator().manual_seed(N + C)
            index = UnitIndex(torch.randn(N, C, generator=g))
            for rows in (1, 16):
                bank = UnitIndexBank([index], device=dev, rows=rows, frames=FRAMES, k=K)
                x = torch.randn(rows, FRAMES, C, generator=g).to(dev)
                which, ratio = torch.zeros(rows, dtype=torch.int32, device=dev), torch.full((rows,), RATIO, device=dev)
                work = x.clone()

                def kernel():
                    work.copy_(x)
                    ctx.units_retrieve_(work, bank, which, ratio, k=K)

                def eager():
                    torch_retrieve(x, bank.vec, K, RATIO)
                t = time_calls({"kernel": kernel, "torch": eager}, repeats)
                torch.cuda.synchronize()
                ctx.poll_error()
                diff = float((work - torch_retrieve(x, bank.vec, K, RATIO)).abs().max())
                floor_ms = N * (C + 1) * 4 / (hbm_tbs * 1e12) * 1e3
                row = {"rows": rows, "frames": FRAMES, "C": C, "N": N, "k": K,
                       **{f"{name}_median_ms": float(np.median(v)) for name, v in t.items()},
                       **{f"{name}_min_ms": float(np.min(v)) for name, v in t.items()},
                       "index_read_ms": floor_ms, "kernel_over_index_read": float(np.median(t["kernel"])) / floor_ms,
                       "max_abs_diff_to_torch": diff, "repeats": repeats}
                print(json.dumps(row), flush=True)
                rows_out.append(row)
                del bank
            del index
            torch.cuda.empty_cache()
    return rows_out


def bank_block(blocks, warmup, entries):
    import numpy as np
    import torch

    import crepe_cases as CC
    import hubert_cases as HC
    import realtime
    import synthetic
    from ddsp.crepe import Crepe
    from ddsp.hubert import HubertSoft
    from ddsp.vocoder import Units_Encoder
    from infer_offline import UnitIndex, UnitIndexBank
    dev = torch.device("cuda:0")
    S, sr, block_time, xfade, buffers = 16, 48000, 0.2, 0.04, 4
    with contextlib.redirect_stdout(sys.stderr), tempfile.TemporaryDirectory() as tmp:
        model = synthetic.build_model("CombSub", seed=1, device=dev)[0]
        crepe = Crepe("full")
        crepe.load_state_dict(CC.fill("full"))
        crepe = crepe.to(dev).eval()
        path = os.path.join(tmp, "hubert-soft.pt")
        torch.save(HC.fill({k: tuple(v.shape) for k, v in HubertSoft().state_dict().items()}), path)
        encoder = Units_Encoder("hubertsoft", path, device=dev)
        kw = dict(buffer_num=buffers, threshold_db=-60.0, use_graph=True, units_encoder=encoder, f0_extractor="crepe", crepe_ckpt=crepe)
        C = int(model.unit2ctrl.n_unit)
        index = UnitIndexBank([UnitIndex(torch.randn(entries, C, generator=torch.Generator().manual_seed(7)))], device=dev)
        banks = {"plain": realtime.StreamBank(model, S, sr, block_time, xfade, dev, **kw),
                 "index": realtime.StreamBank(model, S, sr, block_time, xfade, dev, indices=index, **kw)}
        for s in range(S):
            banks["index"].set_index(s, 0, RATIO)
    block = banks["plain"].block
    rng = np.random.Generator(np.random.PCG64(3))
    t = np.arange(8 * block) / sr
    tones = (147.0, 220.0, 330.0, 196.0)
    rows = [0.2 * np.sin(2 * np.pi * tones[s % 4] * (1 + s // 4) * t) + 0.01 * rng.standard_normal(t.size) for s in range(S)]
    pcm = torch.from_numpy(np.stack(rows).astype(np.float32)).to(dev).reshape(S, 8, block).transpose(0, 1).contiguous()
    times = {name: [] for name in banks}
    for i in range(warmup + blocks):
        for name, bank in banks.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bank.push_audio(pcm[i % 8])
            torch.cuda.synchronize()
            if i >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    row = {"streams": S, "block_ms": block_time * 1e3, "frames": banks["plain"].frames, "C": C, "N": entries, "k": K, "blocks": blocks,
           **{f"{name}_mean_ms": float(np.mean(v)) for name, v in times.items()},
           **{f"{name}_p99_ms": float(np.percentile(v, 99)) for name, v in times.items()}}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieve_time.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bank-entries", type=int, default=10_000)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="the HBM bandwidth the index's read time is quoted at, TB/s (MI355X: 8 peak)")
    ap.add_argument("--skip-bank", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("retrieve_time needs a HIP device")
    doc = {"what": "one units_retrieve_ call against cdist + topk + gather in torch, alternating in one process (HIP events, median "
                   "and fastest of `repeats`); index_read_ms = the index's bytes at hbm_tbs TB/s",
           "device": torch.cuda.get_device_name(0), "hbm_tbs": a.hbm_tbs, "calls": calls(a.repeats, a.hbm_tbs)}
    if not a.skip_bank:
        doc["bank"] = bank_block(a.blocks, a.warmup, a.bank_entries)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
