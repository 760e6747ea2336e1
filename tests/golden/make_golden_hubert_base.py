"""Generates tests/golden/ref_hubert_base.npz: the HuBERT-base form of the units encoder (no input padding, transformer
layer 9, with and without the final projection) on the deterministic weight fill of tests/hubert_cases.py.

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hubert_base.py

The oracle is the REFERENCE's `encoder/hubert/model.py` `Hubert`: `encode(x, layer=9)[0]` on the unpadded audio and `proj(...)`
of it, in fp64 and fp32.  fairseq is not installed, so the mapping of that class's state dict onto fairseq's `HubertModel`
names (tests/hubert_base_cases.py `key_table`) is written down here and stored in the fixture; the tests build fairseq-layout
weights from it.  A second, independent statement of the network is `transformers.HubertModel(HubertConfig())` (the base
architecture, no padding), loaded with the same numbers through the documented fairseq -> transformers names: its fp64
`hidden_states[9]` must agree with the reference class to 1e-9 relative RMS (the same arithmetic in fp64; many orders above
rounding through 9 layers, two orders below any fp32-level difference), or nothing is written.

Stored (fp64 results rounded to fp32):
  map_ref / map_fairseq / map_shapes / map_row0   the key table: fairseq tensor = rows [row0, row0 + shape[0]) of the reference's
  checksums                  per-tensor (sum, sum of squares) of the fill under fairseq's names, in table order
  frames0 / frames0_extra    the reference conv stack's frame counts WITHOUT padding over hubert_cases.FRAME_LENGTHS and
                             hubert_base_cases.EXTRA_FRAME_LENGTHS (-1 where it raises)
  hidden9_64_<case>          the hidden state after 9 transformer layers (B, Fr, 768), fp64; units9_64_<case> its projection
  err32_<case>               the reference's own fp32 error of hidden9 (relative RMS); err32u_<case> of units9
  hf_agree_<case>            relative RMS between transformers' fp64 hidden_states[9] and the reference class's"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden import REF, _placeholders, save  # noqa: E402
import hubert_base_cases as BC  # noqa: E402
import hubert_cases as HC  # noqa: E402

HF_GATE = 1e-9


def hf_names(fs):
    """A fairseq HubertModel key -> its transformers HubertModel key (None: no counterpart in the bare encoder)."""
    if fs in ("label_embs_concat", "final_proj.weight", "final_proj.bias"):
        return None
    if fs == "mask_emb":
        return "masked_spec_embed"
    for a, b in ((".0.0.weight", ".0.conv.weight"), (".0.2.", ".0.layer_norm.")):
        if fs.startswith("feature_extractor.conv_layers.0") and a in fs:
            return fs.replace(a, b)
    if fs.startswith("feature_extractor.conv_layers."):
        return fs.replace(".0.weight", ".conv.weight")
    if fs.startswith("post_extract_proj."):
        return fs.replace("post_extract_proj.", "feature_projection.projection.")
    if fs.startswith("layer_norm."):
        return "feature_projection." + fs
    if fs.startswith("encoder.pos_conv.0."):
        tail = {"bias": "bias", "weight_g": "parametrizations.weight.original0", "weight_v": "parametrizations.weight.original1"}
        return "encoder.pos_conv_embed.conv." + tail[fs.rsplit(".", 1)[1]]
    for a, b in ((".self_attn_layer_norm.", ".layer_norm."), (".self_attn.", ".attention."),
                 (".fc1.", ".feed_forward.intermediate_dense."), (".fc2.", ".feed_forward.output_dense.")):
        if a in fs:
            return fs.replace(a, b)
    return fs      # encoder.layer_norm.*, encoder.layers.i.final_layer_norm.*


def main():
    import warnings
    warnings.simplefilter("ignore")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    # (before the placeholders: transformers probes optional packages by their import spec, which a placeholder lacks)
    from transformers import HubertConfig, HubertModel
    hf = HubertModel(HubertConfig()).eval()
    before = set(sys.modules)
    _placeholders()
    for k in [k for k in sys.modules if k == "ddsp" or k.startswith("ddsp.") or k.startswith("encoder")]:
        del sys.modules[k]
    sys.path.insert(0, REF)
    from encoder.hubert.model import Hubert
    sys.path.remove(REF)
    for k in set(sys.modules) - before:
        if not k.startswith("encoder") and getattr(sys.modules[k], "__spec__", None) is None:
            del sys.modules[k]                       # the placeholders have served the reference's imports

    m32 = Hubert().eval()
    shapes = {k: tuple(v.shape) for k, v in m32.state_dict().items()}
    sd = HC.fill(shapes)
    m32.load_state_dict(sd, strict=True)
    m64 = Hubert().eval()
    m64.load_state_dict(sd, strict=True)
    m64 = m64.double()

    table = BC.key_table(shapes)
    fs_sd = BC.fairseq_state(table, sd)
    out = {"map_ref": np.array([r for r, _, _, _ in table]), "map_fairseq": np.array([f for _, f, _, _ in table]),
           "map_shapes": np.array([str(s) for _, _, s, _ in table]), "map_row0": np.array([o for _, _, _, o in table]),
           "checksums": HC.checksums(fs_sd)}

    def frames(lengths):
        got = []
        with torch.inference_mode():
            for T in lengths:
                try:
                    got.append(m32.feature_extractor(torch.zeros(1, 1, T)).shape[-1])
                except (RuntimeError, ValueError):      # (a one-frame conv0 output is refused by the GroupNorm)
                    got.append(-1)
        return np.array(got)
    out["frames0"], out["frames0_extra"] = frames(HC.FRAME_LENGTHS), frames(BC.EXTRA_FRAME_LENGTHS)

    hf_sd = {hf_names(k): v for k, v in fs_sd.items() if hf_names(k) is not None}
    missing, unexpected = hf.load_state_dict(hf_sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    hf = hf.double()

    with torch.inference_mode():
        for name in BC.CASES:
            x = HC.audio(name).unsqueeze(1)
            h32, h64 = m32.encode(x, layer=9)[0], m64.encode(x.double(), layer=9)[0]
            u32, u64 = m32.proj(h32), m64.proj(h64)
            third = hf(x[:, 0].double(), output_hidden_states=True).hidden_states[9]
            agree = BC.rel(third, h64)
            out[f"hidden9_64_{name}"], out[f"units9_64_{name}"] = h64.float(), u64.float()
            out[f"err32_{name}"], out[f"err32u_{name}"], out[f"hf_agree_{name}"] = BC.rel(h32, h64), BC.rel(u32, u64), agree
            print(name, tuple(h64.shape), "fp32 vs fp64", out[f"err32_{name}"], out[f"err32u_{name}"], "transformers vs reference",
                  agree, flush=True)
            if not agree <= HF_GATE:
                raise SystemExit(f"{name}: transformers' HubertModel and the reference class differ by {agree:.3e} > {HF_GATE:.0e} in "
                                 "fp64: not the same computation; no fixture written")
    save("ref_hubert_base.npz", **out)


if __name__ == "__main__":
    main()
