"""The weight fill of tests/hubert_cases.py under fairseq's HuBERT-base names, shared by the base-form encoder tests and
by tests/golden/make_golden_hubert_base.py, which writes the key table into tests/golden/ref_hubert_base.npz.

The table maps the reference's `Hubert` state dict (tests/golden/ref_hubert_soft.npz: keys, shapes) onto fairseq's
`HubertModel`: every fairseq tensor is rows [row0, row0 + shape[0]) of one reference tensor - the whole of it, except for the
attention's input projections, where nn.MultiheadAttention's `in_proj_weight` (2304, 768) holds q, k and v as three blocks of
768 rows.  So one set of numbers fills a `HubertSoft`, a `HubertBase`, the reference class and any third statement of the
network."""
import numpy as np
import torch

import hubert_cases as HC

CASES = ("short", "odd", "pair")      # of hubert_cases.CASES: `gui` is left out to keep the 768-wide arrays small
# the lengths whose frame count the fixture records beside hubert_cases.FRAME_LENGTHS: the first that gives two frames and
# its neighbours (399 / 400 / 401 are in that list)
EXTRA_FRAME_LENGTHS = [9, 10, 719, 720, 721]


def key_table(ref_shapes):
    """{reference key: shape} -> [(reference key, fairseq key, fairseq shape, row0)] in fairseq's state-dict order."""
    rows = [("masked_spec_embed", "mask_emb", 0), ("label_embedding.weight", "label_embs_concat", 0),
            ("feature_extractor.conv0.weight", "feature_extractor.conv_layers.0.0.weight", 0),
            ("feature_extractor.norm0.weight", "feature_extractor.conv_layers.0.2.weight", 0),
            ("feature_extractor.norm0.bias", "feature_extractor.conv_layers.0.2.bias", 0)]
    rows += [(f"feature_extractor.conv{i}.weight", f"feature_extractor.conv_layers.{i}.0.weight", 0) for i in range(1, 7)]
    rows += [(f"feature_projection.projection.{p}", f"post_extract_proj.{p}", 0) for p in ("weight", "bias")]
    rows += [(f"positional_embedding.conv.{p}", f"encoder.pos_conv.0.{p}", 0) for p in ("bias", "weight_g", "weight_v")]
    for i in range(12):
        r, f = f"encoder.layers.{i}.", f"encoder.layers.{i}."
        for name, block in (("k_proj", 1), ("v_proj", 2), ("q_proj", 0)):
            rows += [(r + "self_attn.in_proj_weight", f + f"self_attn.{name}.weight", block * 768),
                     (r + "self_attn.in_proj_bias", f + f"self_attn.{name}.bias", block * 768)]
        for a, b in (("self_attn.out_proj", "self_attn.out_proj"), ("norm1", "self_attn_layer_norm"), ("linear1", "fc1"),
                     ("linear2", "fc2"), ("norm2", "final_layer_norm")):
            rows += [(r + f"{a}.{p}", f + f"{b}.{p}", 0) for p in ("weight", "bias")]
    rows += [(f"norm.{p}", f"encoder.layer_norm.{p}", 0) for p in ("weight", "bias")]
    rows += [(f"feature_projection.norm.{p}", f"layer_norm.{p}", 0) for p in ("weight", "bias")]
    rows += [(f"proj.{p}", f"final_proj.{p}", 0) for p in ("weight", "bias")]
    out = []
    for ref, fs, row0 in rows:
        shape = tuple(ref_shapes[ref])
        if "in_proj" in ref:
            shape = (768,) + shape[1:]
        out.append((ref, fs, shape, row0))
    return out


def table_of(fix):
    """The key table as the fixture stores it -> [(reference key, fairseq key, shape, row0)]."""
    return [(str(r), str(f), tuple(int(x) for x in str(s).strip("()").split(",") if x.strip()), int(o))
            for r, f, s, o in zip(fix["map_ref"], fix["map_fairseq"], fix["map_shapes"], fix["map_row0"])]


def fairseq_state(table, ref_sd):
    """The key table and a reference-named state dict -> the same numbers as a fairseq-named state dict."""
    return {fs: ref_sd[ref][row0:row0 + shape[0]].clone() for ref, fs, shape, row0 in table}


def fairseq_fill(fix_base, fix_soft):
    """The deterministic fill under fairseq's names, built from the two fixtures alone: the reference's keys and shapes
    (ref_hubert_soft.npz) and the key table (ref_hubert_base.npz).  -> (fairseq state dict, reference-named state dict)"""
    ref_shapes = {str(k): tuple(int(x) for x in str(s).strip("()").split(",") if x.strip())
                  for k, s in zip(fix_soft["keys"], fix_soft["shapes"])}
    ref_sd = HC.fill(ref_shapes)
    return fairseq_state(table_of(fix_base), ref_sd), ref_sd


def rel(a, b):
    a, b = ((x.detach().cpu() if torch.is_tensor(x) else torch.from_numpy(np.asarray(x))).double() for x in (a, b))
    return float(((a - b) ** 2).mean().sqrt() / (b ** 2).mean().sqrt())
