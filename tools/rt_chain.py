"""Per-block time of `realtime.StreamRenderer`'s chain on one GPU (the device half of gui.py's audio callback), mean and p99
over N blocks after warm-up, each block timed from its push to its (block,) output being ready on the device - what the
callback waits for before it copies the block out.

Two shapes: BASELINE config #5 (0.2 s block, buffer 4, 0.04 s cross-fade) and gui.py's Config defaults (1.5 s block, buffer 2,
0.03 s cross-fade), both with a 44.1 kHz CombSub model (seeded random weights), the forward replayed from a HIP graph.
Legs per shape: the model only (44.1 kHz device); a 48 kHz device (fractional-hop volume + 44.1 -> 48 kHz resampling before
the splice); the enhancer at the shipped NSF-HiFiGAN geometry (seeded random weights) with key 0 and with 'auto' (a track
peaking at 1000 Hz: key 5, so the generator runs at a shifted rate between two resamplings); a speaker mix in the graph.

    python tools/rt_chain.py [--blocks N] [--warmup W] [--out result.json]

`--analysis`: the chain from the RAW block, analysis included (CREPE 'full' and HuBERT-Soft with the deterministic weight fills
of tests/crepe_cases.py / tests/hubert_cases.py, 44.1 kHz device, f0 dither on), for both shapes without the enhancer and with
it at key 0, three ways in one process:
  (a) the composition a caller had to write before `push_audio`: eager `F0_Extractor.extract` + `Units_Encoder.encode` on a
      window of its own, then `push_block(block, units=, f0=)` with the synthesis graph;
  (b) `push_audio`, eager;   (c) `push_audio`, the block replayed from one HIP graph.
Three timed rounds per way, interleaved (a, b, c, a, b, c, ...); a row reports the median of the rounds' means and p99s and
their spread (max - min over the rounds).  `--graph-only SHAPE` runs way (c) alone without the enhancer (for a kernel trace).

    python tools/rt_chain.py --analysis [--blocks N] [--warmup W] [--out profiles/rt_audio_chain.json]"""
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
import numpy as np
import torch

import glue_cases as GC
import realtime
import synthetic
from enhancer import Enhancer

SHIPPED = dict(GC.NSF_CONFIG, upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4],
               upsample_initial_channel=512, num_mels=128, hop_size=512, n_fft=2048, win_size=2048)
SHAPES = {"config5": (0.2, 0.04, 4), "gui_defaults": (1.5, 0.03, 2)}
LEGS = {  # name: (device rate, enhancer key (None = off), speaker mix)
    "model": (44100, None, None),
    "device_48k": (48000, None, None),
    "enhancer_key0": (44100, 0, None),
    "enhancer_auto": (44100, "auto", None),
    "mix_graph": (44100, None, {1: 0.3, 3: 0.7}),
}


def shipped_enhancer(dev, tmp):
    with open(os.path.join(tmp, "config.json"), "w") as fh:
        json.dump(SHIPPED, fh)
    torch.save({"generator": GC.nsf_state_dict(SHIPPED, seed=91)}, os.path.join(tmp, "model"))
    with contextlib.redirect_stdout(sys.stderr):
        return Enhancer("nsf-hifigan", os.path.join(tmp, "model"), device=dev)


def time_leg(model, enh, dev, shape, leg, blocks, warmup):
    block_time, xfade_time, buffer_num = SHAPES[shape]
    sr, key, mix = LEGS[leg]
    r = realtime.StreamRenderer(model, sr, block_time, xfade_time, dev, buffer_num=buffer_num, threshold_db=-60.0, spk_id=1,
                                use_graph=True, spk_mix_dict=mix, enhancer=enh if key is not None else None,
                                enhancer_adaptive_key="auto" if key is None else key)
    feat = {k: v.to(dev) for k, v in synthetic.make_inputs(5, 1, r.frames, with_noise=False).items()}
    # a voiced track peaking at 1000 Hz after the enhancer's front cut ('auto' -> key 5)
    f0 = (250.0 + 750.0 * torch.sin(torch.arange(r.frames) / 7.0) ** 2).reshape(1, -1, 1).to(dev)
    rng = np.random.Generator(np.random.PCG64(3))
    pcm = [torch.from_numpy((0.2 * rng.standard_normal(r.block)).astype(np.float32)).to(dev) for _ in range(8)]
    times = []
    for i in range(warmup + blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.push_block(pcm[i % len(pcm)], units=feat["units"], f0=f0)
        torch.cuda.synchronize()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    t = np.array(times)
    return {"shape": shape, "leg": leg, "device_sr": sr, "block_ms": block_time * 1e3, "frames": r.frames,
            "key": r.last_key, "mean_ms": float(t.mean()), "p99_ms": float(np.percentile(t, 99)), "blocks": len(t)}


ROUNDS = 3


def analysis_front(dev, tmp):
    """(Units_Encoder, ddsp.crepe.Crepe 'full') with the deterministic fills of the tests."""
    import crepe_cases as CC
    import hubert_cases as HC
    from ddsp.crepe import Crepe
    from ddsp.hubert import HubertSoft
    from ddsp.vocoder import Units_Encoder
    crepe = Crepe("full")
    crepe.load_state_dict(CC.fill("full"))
    path = os.path.join(tmp, "hubert-soft.pt")
    torch.save(HC.fill({k: tuple(v.shape) for k, v in HubertSoft().state_dict().items()}), path)
    with contextlib.redirect_stdout(sys.stderr):
        return Units_Encoder("hubertsoft", path, device=dev), crepe.to(dev).eval()


def voiced_blocks(block, sr, dev, n=8):
    rng = np.random.Generator(np.random.PCG64(3))
    out = []
    for k in range(n):
        t = (np.arange(block) + k * block) / sr
        x = 0.2 * np.sin(2 * np.pi * 147.0 * t) + 0.01 * rng.standard_normal(block)
        out.append(torch.from_numpy(x.astype(np.float32)).to(dev))
    return out


def audio_ways(model, enh, key, encoder, crepe, dev, shape, which=("a", "b", "c")):
    """{way: push(block) -> emitted block} for one shape, each way on renderers of its own."""
    block_time, xfade_time, buffer_num = SHAPES[shape]
    kw = dict(buffer_num=buffer_num, threshold_db=-60.0, spk_id=1, enhancer=enh if key is not None else None,
              enhancer_adaptive_key=0 if key is None else key)
    front = dict(units_encoder=encoder, f0_extractor="crepe", crepe_ckpt=crepe)
    ways, r0 = {}, None
    if "a" in which:
        plain = r0 = realtime.StreamRenderer(model, 44100, block_time, xfade_time, dev, use_graph=True, **kw)
        from ddsp.vocoder import F0_Extractor
        ex = F0_Extractor("crepe", 44100, plain.hop_size, 50.0, 1100.0, crepe_ckpt=crepe, device=dev)
        state = {"window": torch.zeros(plain.n_in, device=dev)}

        def way_a(blk):
            state["window"] = w = torch.cat([state["window"][plain.block:], blk])
            f0 = ex.extract(w, uv_interp=True, silence_front=plain.silence_front)[None, :, None]
            units = encoder.encode(w[None], 44100, plain.hop_size)
            return plain.push_block(blk, units=units, f0=f0)
        ways["a"] = way_a
    if "b" in which:
        r0 = rb = realtime.StreamRenderer(model, 44100, block_time, xfade_time, dev, use_graph=False, **kw, **front)
        ways["b"] = rb.push_audio
    if "c" in which:
        r0 = rc = realtime.StreamRenderer(model, 44100, block_time, xfade_time, dev, use_graph=True, **kw, **front)
        ways["c"] = rc.push_audio
    return ways, r0


def time_audio(model, enh, key, encoder, crepe, dev, shape, blocks, warmup):
    ways, r = audio_ways(model, enh, key, encoder, crepe, dev, shape)
    pcm = voiced_blocks(r.block, 44100, dev)
    rounds = {w: [] for w in ways}
    for rnd in range(ROUNDS):
        for w, push in ways.items():
            times = []
            for i in range(warmup + blocks):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                push(pcm[i % len(pcm)])
                torch.cuda.synchronize()
                if i >= warmup:
                    times.append((time.perf_counter() - t0) * 1e3)
            t = np.array(times)
            rounds[w].append((float(t.mean()), float(np.percentile(t, 99))))
    names = {"a": "eager analysis + push_block (synthesis graph)", "b": "push_audio eager", "c": "push_audio graph"}
    out = []
    for w, rs in rounds.items():
        means, p99s = [m for m, _ in rs], [p for _, p in rs]
        out.append({"shape": shape, "enhancer_key": key, "way": w, "what": names[w], "block_ms": SHAPES[shape][0] * 1e3,
                    "frames": r.frames, "mean_ms": float(np.median(means)), "p99_ms": float(np.median(p99s)),
                    "mean_spread_ms": max(means) - min(means), "p99_spread_ms": max(p99s) - min(p99s),
                    "rounds": [{"mean_ms": m, "p99_ms": p} for m, p in rs], "blocks_per_round": blocks})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--analysis", action="store_true")
    ap.add_argument("--graph-only", default=None, choices=list(SHAPES))
    a = ap.parse_args()
    if a.blocks is None:
        a.blocks = 100 if a.analysis else 200
    if not torch.cuda.is_available():
        raise SystemExit("rt_chain needs a HIP device")
    dev = torch.device("cuda:0")
    with contextlib.redirect_stdout(sys.stderr):
        model, _ = synthetic.build_model("CombSub", seed=1, device=dev)
    rows = []
    if a.graph_only:
        with tempfile.TemporaryDirectory() as tmp:
            encoder, crepe = analysis_front(dev, tmp)
            ways, r = audio_ways(model, None, None, encoder, crepe, dev, a.graph_only, which=("c",))
            pcm = voiced_blocks(r.block, 44100, dev)
            for i in range(a.warmup + a.blocks):
                ways["c"](pcm[i % len(pcm)])
            torch.cuda.synchronize()
        print(json.dumps({"shape": a.graph_only, "way": "c", "blocks": a.warmup + a.blocks}), flush=True)
        return
    if a.analysis:
        with tempfile.TemporaryDirectory() as tmp:
            enh = shipped_enhancer(dev, tmp)
            encoder, crepe = analysis_front(dev, tmp)
            for shape in SHAPES:
                for key in (None, 0):
                    for row in time_audio(model, enh, key, encoder, crepe, dev, shape, a.blocks, a.warmup):
                        rows.append(row)
                        print(json.dumps({k: v for k, v in row.items() if k != "rounds"}), flush=True)
        out = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "rows": rows}
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(out, fh, indent=1)
        return
    with tempfile.TemporaryDirectory() as tmp:
        enh = shipped_enhancer(dev, tmp)
        for shape in SHAPES:
            for leg in LEGS:
                row = time_leg(model, enh, dev, shape, leg, a.blocks, a.warmup)
                rows.append(row)
                print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
