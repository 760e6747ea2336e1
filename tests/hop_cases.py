"""Cases of the block sizes 128 and 256 (tests/test_gpu_hop.py), shared with the generator of their fixtures
(tests/golden/make_golden_hop.py) and with the CPU test that holds the two together (tests/test_hop_cases_host.py).

Inputs are regenerated from seeds on both sides; the fixtures hold only what the reference computed from them.

FIR cases, (hop, Fr, n, add_in), B = 2 with different rows.  Per hop every Fr of {1, 2, 5, 9} and every n of
{32, 510, 1022, 2046} appears; 9 frames are 1152 samples at hop 128 (4.5 tiles of 256: a partial last tile, and with
n = 2046 several staging batches per block), 2304 at hop 256 (two blocks of 2048 in the forward, three in the input adjoint);
(128, 3, 2046) is a filter longer than the whole signal; (hop, 1, 32) the smallest call there is.
OLA cases, (hop, Fr): Fr = 1 (frame Fr reuses filter 0 and is folded into its adjoint), 2, 5.
Models: B = 2, Fr = 9, small filter banks, one seeded state dict on both sides."""
import numpy as np
import torch

SR = 44100
HOPS = (128, 256)
B = 2

FIR_CASES = [
    (128, 1, 32, False), (128, 2, 510, False), (128, 5, 1022, False), (128, 9, 2046, False), (128, 3, 2046, False),
    (128, 9, 32, True),
    (256, 1, 32, False), (256, 2, 2046, False), (256, 5, 510, False), (256, 9, 1022, True),
]
OLA_CASES = [(hop, Fr) for hop in HOPS for Fr in (1, 2, 5)]
OLA_PAD = 5                      # control stride wider than the three blocks

MODELS = ("CombSub", "Sins", "CombSubFast")
MODEL_FR = 9
MODEL_RAGGED = [9, 4]
MODEL_KW = {
    "CombSub": dict(n_mag_allpass=65, n_mag_harmonic=128, n_mag_noise=65),
    "Sins": dict(n_harmonics=32, n_mag_allpass=65, n_mag_noise=65),
    "CombSubFast": dict(),
}
N_UNIT, N_SPK = 256, 100
WEIGHT_SEED, INPUT_SEED, TARGET_SEED = 4107, 4111, 4113
# RSSLoss(fft_min, fft_max, n_scale) of the training case and the scales it is held to: below 9 * 128 samples
LOSS_RANGE = (256, 1024, 4)
LOSS_SCALES = [300, 517, 777, 1023]


def fir_id(c):
    return "hop%d-Fr%d-n%d%s" % (c[0], c[1], c[2], "-add" if c[3] else "")


def ola_id(c):
    return "hop%d-Fr%d" % c


def fir_key(c, what):
    return f"{what}_{c[0]}_{c[1]}_{c[2]}"


def ola_key(c, what):
    return f"{what}_{c[0]}_{c[1]}"


def model_key(name, hop, what):
    return f"{name}_{hop}_{what}"


def fir_inputs(case):
    """x ~ U(-1, 1) (B, T), ir ~ N(0, 1/n) (B, Fr, n) - the scale of tests/test_gpu_dsp.py::test_ltv_fir_small_vs_direct -,
    upstream gradient g ~ N(0, 1) (B, T), add ~ N(0, 1) (B, T)."""
    hop, Fr, n, _ = case
    rng = np.random.Generator(np.random.PCG64(100000 * hop + 10 * n + Fr))
    T = Fr * hop
    x = torch.from_numpy(rng.uniform(-1, 1, size=(B, T)).astype(np.float32))
    ir = torch.from_numpy((rng.standard_normal((B, Fr, n)) / np.sqrt(n)).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((B, T)).astype(np.float32))
    add = torch.from_numpy(rng.standard_normal((B, T)).astype(np.float32))
    return x, ir, g, add


def ola_inputs(case):
    """ctrl ~ N(0, 0.25) (B*Fr, 3*(hop+1) + OLA_PAD), comb ~ U(-1, 1), unit noise u on the 24-bit grid, g ~ N(0, 1)."""
    hop, Fr = case
    rng = np.random.Generator(np.random.PCG64(7000 + 10 * hop + Fr))
    T = Fr * hop
    ctrl = torch.from_numpy((rng.standard_normal((B * Fr, 3 * (hop + 1) + OLA_PAD)) * 0.5).astype(np.float32))
    comb = torch.from_numpy(rng.uniform(-1, 1, (B, T)).astype(np.float32))
    u = torch.from_numpy(rng.random((B, T), dtype=np.float32))
    g = torch.from_numpy(rng.standard_normal((B, T)).astype(np.float32))
    return ctrl, comb, u, g


def build_model(name, hop, device="cpu"):
    """The product's class at block size `hop` with seeded weights (reference state-dict shapes)."""
    from ddsp.vocoder import CombSub, CombSubFast, Sins
    state = torch.random.get_rng_state()
    torch.manual_seed(WEIGHT_SEED)
    try:
        kw = MODEL_KW[name]
        if name == "CombSub":
            m = CombSub(SR, hop, kw["n_mag_allpass"], kw["n_mag_harmonic"], kw["n_mag_noise"], N_UNIT, N_SPK)
        elif name == "Sins":
            m = Sins(SR, hop, kw["n_harmonics"], kw["n_mag_allpass"], kw["n_mag_noise"], N_UNIT, N_SPK)
        else:
            m = CombSubFast(SR, hop, N_UNIT, N_SPK)
    finally:
        torch.random.set_rng_state(state)
    return m.to(device).eval()


def model_inputs(hop):
    import synthetic
    return synthetic.make_inputs(INPUT_SEED + hop, B, MODEL_FR, n_unit=N_UNIT, n_spk=N_SPK, hop=hop)


def train_target(hop):
    rng = np.random.Generator(np.random.PCG64(TARGET_SEED + hop))
    return torch.from_numpy((0.1 * rng.standard_normal((B, MODEL_FR * hop))).astype(np.float32))
