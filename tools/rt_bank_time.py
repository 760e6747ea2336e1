"""Per-block time of `realtime.StreamBank.push_audio` (S streams, one graph replay) against S solo `StreamRenderer`s of a
BASELINE checkout pushed one after the other, each with its own captured graph: what one GPU pays per block period for S
callers, before and after the bank.

Geometry: the two timings `config5` (0.2 s blocks, buffer 4, 0.04 s cross-fade) and `gui` (1.5 s blocks, buffer 2, 0.03 s
cross-fade) on a 48 kHz device (fractional-hop volume and the 44.1 -> 48 kHz resampler are in the chain), a 44.1 kHz CombSub
(seeded random weights), CREPE 'full' and HuBERT-Soft with the deterministic fills of tests/crepe_cases.py / tests/hubert_cases.py,
f0 dither on.  Cases: S in {1, 4, 16}.  Per case mean / p99 over `--blocks` blocks after `--warmup`, each block timed from the
push to the (S, block) output being ready on the device.

The two legs load different builds of the library, so each runs in a fresh process of its own: `bank` imports the package of
THIS tree, `solo` the package of `--baseline-tree`.  The legs alternate `--repeats` times in one session
(bank, solo, bank, solo, ...), every process under its own `timeout`; a leg that ends abnormally ends the session.  Every
repeat is written out; nothing is averaged away.

`--enhancer` puts the NSF-HiFiGAN enhancer at the shipped generator geometry (seeded random weights, as tools/rt_chain.py builds
it) with `enhancer_adaptive_key='auto'` into both legs, for the `config5` timing only: the bank runs it as its captured keyed
stage, every solo renderer eagerly with its one read-back per block.  The solo leg needs nothing the parent commit lacks, so
`--baseline-tree` may then be left out (both legs import this tree).

    python tools/rt_bank_time.py --baseline-tree <parent checkout> [--blocks 200] [--warmup 10] [--shapes config5]
                                 [--out profiles/rt_bank_time.json]
    python tools/rt_bank_time.py --enhancer [--out profiles/rt_bank_enhancer_time.json]

`--active A` times a bank of S slots of which A are active: the bank leg builds its banks with `active_widths=(A,)` and pushes
(A, block) blocks with `active=` (A slots spread evenly over the S), the solo leg pushes A solo renderers; cases with S < A are
left out, and every row carries `"active": A`.

`--models M` times a bank whose S slots are dealt round-robin over M distinct models (CombSub, seeds 1..M): the bank leg builds
`StreamBank(models=...)` with the default `model_widths` and gives slot s model s % M, the solo leg pushes S solo renderers of
the baseline tree, renderer s over model s % M - the only way the parent commit serves M models.  With M = 1 a third leg,
`plain`, times the ordinary single-model bank of this tree beside the one-model bank that goes through the per-model path.
Cases with S < M are left out; `--streams` picks the S to run; every row carries `"models": M`.  Combines with `--enhancer` and
`--active`.

    python tools/rt_bank_time.py --baseline-tree <parent checkout> --models 4 --streams 16 --shapes config5
                                 [--out profiles/rt_bank_models_time.json]

`--glide` times what a voice that glides costs a bank: three legs, all banks, alternating as above - `parent`, the bank of the
baseline tree; `plain`, the bank of this tree built without `glide_breakpoints` (the same launches as the parent's: a difference
beyond the session's run-to-run spread is a finding); `glide`, the bank of this tree with `glide_breakpoints=4` and a timeline on
every slot that ramps through the whole run (one more launch per block, and the per-frame weights in the prenet's epilogue).

    python tools/rt_bank_time.py --baseline-tree <parent checkout> --glide --streams 16 --shapes config5
                                 [--out profiles/rt_bank_glide_time.json]

`--pitch-glide` times what a key that glides costs a bank, the same way: `parent`, the bank of the baseline tree; `unused`, the
bank of this tree with `pitch_breakpoints=4` and no timeline set (one more launch per block, which copies each slot's one
factor to its frames); `pitch`, the same bank with a key timeline on every slot that ramps through the whole run.

    python tools/rt_bank_time.py --baseline-tree <parent checkout> --pitch-glide --streams 16 --shapes config5
                                 [--out profiles/rt_bank_pitch_time.json]

`--tune` times what pitch correction costs a bank, the same way: `parent`, the bank of the baseline tree; `plain`, the bank of
this tree built without `tune=True` (the same launches as the parent's); `tune`, the bank of this tree with `tune=True` and a
scale on every slot (one more launch per block, `ddsp_f0_tune`, inside the captured block).

    python tools/rt_bank_time.py --baseline-tree <parent checkout> --tune --streams 16 --shapes config5
                                 [--out profiles/rt_bank_tune_time.json]"""
import argparse
import contextlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"config5": (0.2, 0.04, 4), "gui": (1.5, 0.03, 2)}
STREAMS = (1, 4, 16)
DEVICE_SR = 48000
TONES = (147.0, 220.0, 330.0, 196.0)


SHIPPED_NSF = dict(upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4], upsample_initial_channel=512,
                   num_mels=128, hop_size=512, n_fft=2048, win_size=2048)


def leg(which, tree, blocks, warmup, with_enhancer=False, shapes=tuple(SHAPES), active=None, models=None, streams=STREAMS):
    """One leg in this process: `which` = 'bank' | 'solo' | 'plain' | 'parent' | 'glide' | 'unused' | 'pitch' | 'tune', the package taken from `tree`.  Prints one
    JSON row per case."""
    sys.path.insert(0, os.path.join(tree, "ddsp-svc-official_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch

    import crepe_cases as CC
    import hubert_cases as HC
    import realtime
    import synthetic
    from ddsp.crepe import Crepe
    from ddsp.hubert import HubertSoft
    from ddsp.vocoder import Units_Encoder
    if not torch.cuda.is_available():
        raise SystemExit("rt_bank_time needs a HIP device")
    dev = torch.device("cuda:0")
    with contextlib.redirect_stdout(sys.stderr), tempfile.TemporaryDirectory() as tmp:
        pool = [synthetic.build_model("CombSub", seed=1 + k, device=dev)[0] for k in range(models or 1)]
        model = pool[0]
        crepe = Crepe("full")
        crepe.load_state_dict(CC.fill("full"))
        crepe = crepe.to(dev).eval()
        path = os.path.join(tmp, "hubert-soft.pt")
        torch.save(HC.fill({k: tuple(v.shape) for k, v in HubertSoft().state_dict().items()}), path)
        encoder = Units_Encoder("hubertsoft", path, device=dev)
        enh = None
        if with_enhancer:
            import glue_cases as GC
            from enhancer import Enhancer
            cfg = dict(GC.NSF_CONFIG, **SHIPPED_NSF)
            with open(os.path.join(tmp, "config.json"), "w") as fh:
                json.dump(cfg, fh)
            torch.save({"generator": GC.nsf_state_dict(cfg, seed=91)}, os.path.join(tmp, "model"))
            enh = Enhancer("nsf-hifigan", os.path.join(tmp, "model"), device=dev)
    for shape, (block_time, xfade_time, buffer_num) in SHAPES.items():
        if shape not in shapes or (with_enhancer and shape != "config5"):
            continue
        for S in streams:
            if (active is not None and S < active) or (models is not None and S < models):
                continue
            A = S if active is None else active
            slots = None if active is None else [(r * S) // A for r in range(A)]
            kw = dict(buffer_num=buffer_num, threshold_db=-60.0, use_graph=True, units_encoder=encoder, f0_extractor="crepe",
                      crepe_ckpt=crepe)
            if with_enhancer:
                kw.update(enhancer=enh, enhancer_adaptive_key="auto")
            with contextlib.redirect_stdout(sys.stderr):
                if which != "solo":
                    if active is not None:
                        kw.update(active_widths=(A,))
                    if models is not None and which == "bank":
                        kw.update(models=pool)
                    if which == "glide":
                        kw.update(glide_breakpoints=4)
                    if which in ("unused", "pitch"):
                        kw.update(pitch_breakpoints=4)
                    if which == "tune":
                        kw.update(tune=True)
                    bank = realtime.StreamBank(model, S, DEVICE_SR, block_time, xfade_time, dev, **kw)
                    if which == "tune":     # every slot in a scale of its own, at 50 ms
                        from infer_offline import PitchTune
                        for s in range(S):
                            bank.set_tune(s, PitchTune.scale(s % 12, ("major", "minor", "major_pentatonic")[s % 3]))
                    for s in range(S if "models" in kw else 0):
                        bank.set_model(s, s % len(pool))
                    if which == "glide":    # every slot ramps between two voices for the whole run, each at its own pace
                        from infer_offline import SpeakerTimeline
                        span = (warmup + blocks) * block_time
                        for s in range(S):
                            at = [span * n / (3 + s % 3) for n in range(4)]
                            bank.set_timeline(s, SpeakerTimeline([(t, {1 + s % 7: 1.0 - n % 2, 8 + s % 5: float(n % 2)}) for n, t in enumerate(at)]))
                    if which == "pitch":    # every slot's key ramps up and down for the whole run, each at its own pace
                        from infer_offline import KeyTimeline
                        span = (warmup + blocks) * block_time
                        for s in range(S):
                            at = [span * n / (3 + s % 3) for n in range(4)]
                            bank.set_pitch_timeline(s, KeyTimeline([(t, (-3.0, 4.0)[n % 2] + s % 5) for n, t in enumerate(at)]))
                    block, frames = bank.block, bank.frames
                    push = bank.push_audio if active is None else (lambda blocks: bank.push_audio(blocks, active=slots))
                else:
                    owners = range(S) if slots is None else slots
                    solo = [realtime.StreamRenderer(pool[s % len(pool)], DEVICE_SR, block_time, xfade_time, dev, spk_id=1, **kw)
                            for s in owners]
                    block, frames = solo[0].block, solo[0].frames

                    def push(blocks):
                        return [r.push_audio(blocks[s]) for s, r in enumerate(solo)]
            rng = np.random.Generator(np.random.PCG64(3))
            t = np.arange(8 * block) / DEVICE_SR
            rows = [0.2 * np.sin(2 * np.pi * TONES[s % len(TONES)] * (1 + s // len(TONES)) * t) + 0.01 * rng.standard_normal(t.size)
                    for s in range(A)]
            pcm = torch.from_numpy(np.stack(rows).astype(np.float32)).to(dev).reshape(A, 8, block).transpose(0, 1).contiguous()
            times = []
            for i in range(warmup + blocks):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                push(pcm[i % 8])
                torch.cuda.synchronize()
                if i >= warmup:
                    times.append((time.perf_counter() - t0) * 1e3)
            ts = np.array(times)
            print(json.dumps({**({} if active is None else {"active": A}), **({} if models is None else {"models": models}), "leg": which, "shape": shape, "streams": S, "enhancer": bool(with_enhancer), "block_ms": block_time * 1e3, "frames": frames,
                              "mean_ms": float(ts.mean()), "p99_ms": float(np.percentile(ts, 99)), "blocks": len(ts),
                              "device": torch.cuda.get_device_name(0)}), flush=True)
            del push
            if which != "solo":
                del bank
            else:
                del solo
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--blocks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds one leg's process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_bank_time.json"))
    ap.add_argument("--enhancer", action="store_true", help="both legs with the NSF-HiFiGAN enhancer, key 'auto' (config5 only)")
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES), help="the timings to run (default: both)")
    ap.add_argument("--active", type=int, default=None, help="time banks of S slots with this many active rows (S >= A only)")
    ap.add_argument("--models", type=int, default=None, help="deal the S slots round-robin over this many distinct models (S >= M only)")
    ap.add_argument("--streams", type=int, nargs="+", default=list(STREAMS), help="the stream counts S to run")
    ap.add_argument("--glide", action="store_true", help="three bank legs: the parent's, this tree's without and with a glide on every slot")
    ap.add_argument("--pitch-glide", action="store_true", help="three bank legs: the parent's, this tree's with pitch_breakpoints unused and with a "
                    "key timeline on every slot")
    ap.add_argument("--tune", action="store_true", help="three bank legs: the parent's, this tree's without tune=True and with a scale on every slot")
    ap.add_argument("--leg", default=None, choices=["bank", "solo", "plain", "parent", "glide", "unused", "pitch", "tune"], help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.tree, a.blocks, a.warmup, a.enhancer, a.shapes, a.active, a.models, a.streams)
    if a.enhancer and not a.baseline_tree:
        a.baseline_tree = ROOT
    if not a.baseline_tree or not os.path.isdir(os.path.join(a.baseline_tree, "ddsp-svc-official_amd")):
        raise SystemExit("rt_bank_time: --baseline-tree must be a checkout of the parent commit (with ddsp-svc-official_amd/)")
    if a.glide and (a.models or a.enhancer):
        raise SystemExit("rt_bank_time: --glide does not combine with --models (such a bank refuses a glide) or --enhancer")
    if a.pitch_glide and (a.glide or a.models or a.enhancer):
        raise SystemExit("rt_bank_time: --pitch-glide is a run of its own (no --glide, --models or --enhancer)")
    if a.tune and (a.glide or a.pitch_glide or a.models or a.enhancer):
        raise SystemExit("rt_bank_time: --tune is a run of its own (no --glide, --pitch-glide, --models or --enhancer)")
    three = ("parent", "plain", "glide") if a.glide else ("parent", "unused", "pitch") if a.pitch_glide else \
        ("parent", "plain", "tune") if a.tune else None
    trees = {"tune": ROOT, "bank": ROOT, "plain": ROOT, "glide": ROOT, "unused": ROOT, "pitch": ROOT, "solo": os.path.abspath(a.baseline_tree), "parent": os.path.abspath(a.baseline_tree)}
    legs = three if three else ("bank", "solo", "plain") if a.models == 1 else ("bank", "solo")
    repeats = []
    for rep in range(a.repeats):
        for which in legs:
            cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", which, "--tree",
                   trees[which], "--blocks", str(a.blocks), "--warmup", str(a.warmup)] + (["--enhancer"] if a.enhancer else []) + \
                  (["--active", str(a.active)] if a.active else []) + (["--models", str(a.models)] if a.models else []) + \
                  ["--streams", *map(str, a.streams)] + ["--shapes", *a.shapes]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:   # a fault, an abort or the time limit: nothing more is started on the device
                raise SystemExit(f"rt_bank_time: leg {which} of repeat {rep} ended with status {p.returncode}; stopping")
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    row = dict(json.loads(line), repeat=rep)
                    repeats.append(row)
                    print(json.dumps(row), flush=True)
    # per case: every repeat's mean, the spread of each leg between its repeats, the S-fold solo time against the bank
    cases = []
    for shape in (["config5"] if a.enhancer else a.shapes):
        for S in a.streams:
            if (a.active is not None and S < a.active) or (a.models is not None and S < a.models):
                continue
            pick = lambda which, key: [r[key] for r in repeats if (r["leg"], r["shape"], r["streams"]) == (which, shape, S)]
            med = lambda v: sorted(v)[len(v) // 2]
            if three:     # three banks: every repeat's mean, each leg's median and spread, and the two differences of the medians
                case = {"shape": shape, "streams": S}
                for which in legs:
                    m = pick(which, "mean_ms")
                    case.update({f"{which}_mean_ms": m, f"{which}_p99_ms": pick(which, "p99_ms"), f"{which}_median_ms": med(m),
                                 f"{which}_spread_ms": max(m) - min(m)})
                case.update({f"{three[1]}_minus_{three[0]}_ms": case[f"{three[1]}_median_ms"] - case[f"{three[0]}_median_ms"],
                             f"{three[2]}_minus_{three[1]}_ms": case[f"{three[2]}_median_ms"] - case[f"{three[1]}_median_ms"]})
                cases.append(case)
                continue
            bm, sm = pick("bank", "mean_ms"), pick("solo", "mean_ms")
            cases.append({"shape": shape, "streams": S, "bank_mean_ms": bm, "solo_mean_ms": sm, "bank_p99_ms": pick("bank", "p99_ms"),
                          "solo_p99_ms": pick("solo", "p99_ms"), "bank_spread_ms": max(bm) - min(bm),
                          "solo_spread_ms": max(sm) - min(sm), "bank_median_ms": med(bm), "solo_median_ms": med(sm),
                          "solo_over_bank": med(sm) / med(bm)})
            if "plain" in legs:   # the single-model bank of this tree beside the one-model bank through the per-model path
                pm = pick("plain", "mean_ms")
                cases[-1].update(plain_mean_ms=pm, plain_median_ms=med(pm), plain_spread_ms=max(pm) - min(pm))
    what = "ms per block period for all S streams: bank = one StreamBank.push_audio; solo = S StreamRenderer.push_audio of the " \
           "baseline tree one after the other"
    if a.glide:
        what = "ms per block period of one StreamBank.push_audio for all S streams: parent = the baseline tree's bank; plain = this " \
               "tree's bank without glide_breakpoints; glide = this tree's bank with glide_breakpoints=4 and a timeline on every slot"
    if a.pitch_glide:
        what = "ms per block period of one StreamBank.push_audio for all S streams: parent = the baseline tree's bank; unused = this " \
               "tree's bank with pitch_breakpoints=4 and no timeline; pitch = the same bank with a key timeline on every slot"
    if a.tune:
        what = "ms per block period of one StreamBank.push_audio for all S streams: parent = the baseline tree's bank; plain = this " \
               "tree's bank without tune=True; tune = this tree's bank with tune=True and a scale on every slot"
    out = {**({} if a.active is None else {"active": a.active}), **({} if a.models is None else {"models": a.models}),
           **({"glide": True} if a.glide else {}), **({"pitch_glide": True} if a.pitch_glide else {}), **({"tune": True} if a.tune else {}), "enhancer": bool(a.enhancer), "device_sr": DEVICE_SR, "blocks": a.blocks,
           "warmup": a.warmup, "repeats": a.repeats, "what": what, "cases": cases, "rows": repeats}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    for c in cases if three else ():
        print(f"{c['shape']:8s} S={c['streams']:2d}: " + ", ".join(f"{w} {c[w + '_median_ms']:.3f} ms (spread {c[w + '_spread_ms']:.3f})" for w in legs) +
              f"; {three[1]} - {three[0]} {c[f'{three[1]}_minus_{three[0]}_ms']:+.3f} ms, "
              f"{three[2]} - {three[1]} {c[f'{three[2]}_minus_{three[1]}_ms']:+.3f} ms")
    for c in () if three else cases:
        print(f"{c['shape']:8s} S={c['streams']:2d}: bank {c['bank_median_ms']:8.3f} ms (spread {c['bank_spread_ms']:.3f}), "
              f"solo x S {c['solo_median_ms']:8.3f} ms (spread {c['solo_spread_ms']:.3f}), ratio {c['solo_over_bank']:.2f}")


if __name__ == "__main__":
    main()
