"""Time per output sample of `ddsp_ltv_fir` and `ddsp_spectral_ola` at hop 128, 256 and 512.
B = 64 rows of two seconds at 44.1 kHz (88064 samples: 688 / 344 / 172 frames), the filter lengths of the shipped CombSub
(n = 510: all-pass and noise, n = 1022: harmonic).  Device events around `reps` calls after a warm-up, three rounds per
figure with the hops alternating inside a round; prints one JSON line (min and max of the rounds, ns per sample).
Usage: python tools/hop_time.py [reps]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ddsp-svc-official_amd"))
import torch      # noqa: E402
import hipddsp    # noqa: E402

dev = torch.device("cuda:0")
ctx = hipddsp.context_for(dev)
B, T = 64, 88064
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
HOPS = (128, 256, 512)


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e6 / (B * T)      # ns per output sample


def cases():
    x = torch.rand(B, T, device=dev) * 2 - 1
    u = torch.rand(B, T, device=dev)
    out = {}
    for hop in HOPS:
        Fr = T // hop
        for n in (510, 1022):
            ir = torch.randn(B, Fr, n, device=dev) / n ** 0.5
            out[f"fir_fp32_n{n}_hop{hop}"] = lambda ir=ir, Fr=Fr, hop=hop: ctx.ltv_fir(x, ir, B, Fr, hop, math=hipddsp.FIR_FP32)
            if hop == 512:
                out[f"fir_split_bf16_n{n}_hop{hop}"] = lambda ir=ir, Fr=Fr, hop=hop: ctx.ltv_fir(x, ir, B, Fr, hop,
                                                                                                  math=hipddsp.FIR_SPLIT_BF16)
        ctrl = torch.randn(B * Fr, 3 * (hop + 1), device=dev) * 0.5
        out[f"ola_hop{hop}"] = lambda ctrl=ctrl, Fr=Fr, hop=hop: ctx.spectral_ola(ctrl, x, u, hipddsp.EXC_UNIT_NOISE, 0, B, Fr, hop)
    return out


if __name__ == "__main__":
    fns = cases()
    rounds = [{k: timed(f) for k, f in fns.items()} for _ in range(3)]
    print(json.dumps({"device": torch.cuda.get_device_name(0), "B": B, "T": T, "reps": reps, "unit": "ns per output sample",
                      "min_max": {k: [round(min(r[k] for r in rounds), 4), round(max(r[k] for r in rounds), 4)] for k in fns}}))
