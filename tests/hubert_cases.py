"""Weights, audio and shapes of tests/golden/ref_hubert_soft.npz (tests/golden/make_golden_hubert.py), shared by the
HuBERT-Soft encoder tests.

The weight fill is deterministic and independent of torch's generator: per state-dict key, numpy's default generator seeded
with the CRC-32 of the key draws N(0, 1) values, scaled as
  norm gains (1-D `...norm*.weight`)   1 + 0.1 N
  biases and other 1-D vectors         0.02 N
  `weight_g` (the weight-norm gains)   |1 + 0.1 N|
  every other weight                   N / sqrt(fan_in), fan_in = the numel of one output row."""
import zlib

import numpy as np
import torch

# name -> (B, T, audio seed): 0.5 s, a length that is not a multiple of the 320-sample hop, the GUI window
# ((1 + buffer_num) * block_time = 4.5 s at 16 kHz), and a batch of two utterances of equal length
CASES = {"short": (1, 8000, 11), "odd": (1, 23457, 12), "gui": (1, 72000, 13), "pair": (2, 16000, 14)}
# lengths whose conv-stack frame count the fixture records (-1: the reference's conv stack rejects the audio)
FRAME_LENGTHS = [0, 100, 319, 320, 321, 399, 400, 401, 480, 8000, 23457, 72000]
# the Units_Encoder.encode case: the "short" audio at 16 kHz aligned to a 160-sample hop
ENCODE_HOP = 160


def fill_one(key, shape):
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    n = rng.standard_normal(shape)
    if len(shape) == 1 and "norm" in key and key.endswith("weight"):
        a = 1.0 + 0.1 * n
    elif len(shape) == 1:
        a = 0.02 * n
    elif key.endswith("weight_g"):
        a = np.abs(1.0 + 0.1 * n)
    else:
        a = n / np.sqrt(int(np.prod(shape[1:])))
    return a.astype(np.float32)


def fill(shapes):
    """{key: shape} -> {key: float32 tensor}"""
    return {k: torch.from_numpy(fill_one(k, tuple(s))) for k, s in shapes.items()}


def checksums(sd):
    """{key: tensor} -> (n, 2) float64: the sum and the sum of squares of every tensor, in key order."""
    return np.array([[float(v.double().sum()), float((v.double() ** 2).sum())] for v in sd.values()])


def audio(name):
    B, T, seed = CASES[name]
    return torch.from_numpy((0.1 * np.random.default_rng(seed).standard_normal((B, T))).astype(np.float32))


def eager_units(sd, wav):
    """The same network restated in PyTorch functional ops (eager, the products of the tensors' device and dtype): wav
    (B, T) -> units (B, Fr, 256).  `sd` holds the HubertSoft state dict.  The baseline of tools/hubert_time.py and a
    cross-check of the fixture's semantics."""
    import torch.nn.functional as F
    p = lambda k: sd[k]  # noqa: E731
    x = F.pad(wav.unsqueeze(1), (40, 40))
    x = F.conv1d(x, p("feature_extractor.conv0.weight"), stride=5)
    x = F.gelu(F.group_norm(x, 512, p("feature_extractor.norm0.weight"), p("feature_extractor.norm0.bias"), 1e-5))
    for i in range(1, 7):
        x = F.gelu(F.conv1d(x, p(f"feature_extractor.conv{i}.weight"), stride=2))
    x = x.transpose(1, 2)
    x = F.layer_norm(x, (512,), p("feature_projection.norm.weight"), p("feature_projection.norm.bias"), 1e-5)
    x = F.linear(x, p("feature_projection.projection.weight"), p("feature_projection.projection.bias"))
    v, g = p("positional_embedding.conv.weight_v"), p("positional_embedding.conv.weight_g")
    w = v * (g / v.norm(dim=(0, 1), keepdim=True))
    pos = F.conv1d(x.transpose(1, 2), w, p("positional_embedding.conv.bias"), padding=64, groups=16)[..., :-1]
    x = F.layer_norm(x + F.gelu(pos).transpose(1, 2), (768,), p("norm.weight"), p("norm.bias"), 1e-5)
    B, L, _ = x.shape
    for i in range(12):
        q = f"encoder.layers.{i}."
        qkv = F.linear(x, p(q + "self_attn.in_proj_weight"), p(q + "self_attn.in_proj_bias"))
        heads = [t.reshape(B, L, 12, 64).transpose(1, 2) for t in qkv.split(768, dim=-1)]
        att = torch.softmax(heads[0] @ heads[1].transpose(-1, -2) / 8.0, dim=-1) @ heads[2]
        att = F.linear(att.transpose(1, 2).reshape(B, L, 768), p(q + "self_attn.out_proj.weight"), p(q + "self_attn.out_proj.bias"))
        x = F.layer_norm(x + att, (768,), p(q + "norm1.weight"), p(q + "norm1.bias"), 1e-5)
        h = F.linear(F.gelu(F.linear(x, p(q + "linear1.weight"), p(q + "linear1.bias"))), p(q + "linear2.weight"), p(q + "linear2.bias"))
        x = F.layer_norm(x + h, (768,), p(q + "norm2.weight"), p(q + "norm2.bias"), 1e-5)
    return F.linear(x, p("proj.weight"), p("proj.bias"))
