"""Ragged batches, host side (no GPU): `n_frames=` is checked before any device work, the grouping rule of
`infer_offline.render(batch_frames=)` as a pure function, `sharding.RaggedPlan.render_local` with a stub model."""
import numpy as np
import pytest
import torch

import synthetic


@pytest.mark.parametrize("name", ["CombSub", "Sins", "CombSubFast"])
def test_bad_n_frames_raise_before_any_device_work(name):
    """CPU tensors: a valid call would end in the 'HIP device only' RuntimeError; a bad n_frames must be refused first."""
    model, cfg = synthetic.build_model(name, seed=3)
    inp = synthetic.make_inputs(5, 3, 8)
    args = (inp["units"], inp["f0"], inp["volume"], inp["spk_id"])
    bad = [[8, 8], [8, 8, 8, 8], [0, 8, 8], [8, 9, 8], [8, -1, 8], [8.0, 8, 8], [True, 8, 8], 8, "888",
           torch.tensor([8.0, 8.0, 8.0]), torch.tensor([[8, 8, 8]]), torch.tensor([8, 8]), np.array([8, 8, 12])]
    for n in bad:
        with torch.no_grad(), pytest.raises(ValueError):
            model(*args, n_frames=n)
        with pytest.raises(ValueError):       # and before the inference-only refusal
            model(*args, n_frames=n)
    with torch.no_grad(), pytest.raises(ValueError):
        model.unit2ctrl.forward_flat(inp["units"], inp["f0"], inp["volume"], inp["volume"], inp["spk_id"], n_frames=[8, 8, 0])
    # a good one gets past the check, in every accepted form: to the inference-only refusal under grad mode ...
    for n in ([8, 3, 1], (8, 3, 1), torch.tensor([8, 3, 1]), torch.tensor([8, 3, 1], dtype=torch.int32), np.array([8, 3, 1])):
        with pytest.raises(NotImplementedError, match="inference only"):
            model(*args, n_frames=n)
        # ... and without it to the device check (there is no CPU path)
        with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
            model(*args, n_frames=n)


def test_forward_signatures():
    """The public entries of the synthesisers and of the control network keep their parameter lists and defaults."""
    import inspect
    from ddsp.unit2control import Unit2Control
    from ddsp.vocoder import CombSub, CombSubFast, Sins
    P = inspect.Parameter
    req = lambda n: P(n, P.POSITIONAL_OR_KEYWORD)
    opt = lambda n, d=None: P(n, P.POSITIONAL_OR_KEYWORD, default=d)
    head = [req("self"), req("units_frames"), req("f0_frames"), req("volume_frames"), req("spk_id"), opt("spk_mix_dict"),
            opt("initial_phase"), opt("infer", True)]
    tail = [opt("noise"), opt("noise_seed"), opt("n_frames"), opt("spk_mix_rows")]
    kwargs = [P("kwargs", P.VAR_KEYWORD)]
    frames = [req("self"), req("units"), req("f0"), req("phase"), req("volume"), req("spk_id")]
    want = {CombSub.forward: head + tail + kwargs,
            Sins.forward: head + [opt("max_upsample_dim", 32)] + tail,
            CombSubFast.forward: head + tail + kwargs,
            Unit2Control.forward_flat: frames + [opt("spk_mix_dict"), opt("n_frames"), opt("spk_mix_rows")],
            Unit2Control.forward_ragged: [req("self"), req("ctx")] + frames[1:] + [req("spk_mix_dict"), req("n_dev"),
                                                                                   opt("hold", True), opt("spk_mix_rows")],
            Unit2Control.forward_flat_keep: frames + [opt("spk_mix_dict"), opt("ctx")]}
    for f, params in want.items():
        assert list(inspect.signature(f).parameters.values()) == params, f.__qualname__


def test_group_segments_rule():
    from infer_offline import group_segments
    rng = np.random.Generator(np.random.PCG64(11))
    for trial in range(50):
        lengths = [int(x) for x in rng.integers(1, 1300, size=int(rng.integers(1, 40)))]
        bound = int(rng.integers(1, 5000))
        groups = group_segments(lengths, bound)
        assert sorted(i for g in groups for i in g) == list(range(len(lengths)))       # every segment exactly once
        for g in groups:
            padded = len(g) * max(lengths[i] for i in g)
            assert padded <= bound or len(g) == 1, (g, padded, bound)
            assert lengths[g[0]] == max(lengths[i] for i in g)                            # the longest leads its group
    assert group_segments([40, 173, 9, 260, 88], 400) == [[3], [1, 4], [0, 2]]
    assert group_segments([5, 5, 5], 1) == [[0], [1], [2]]
    assert group_segments([], 100) == []
    assert group_segments([7, 7, 7, 7], 28) == [[0, 1, 2, 3]]


class _StubModel:
    """signal[b, t] = 1000 * (units[b, t // hop, 0]) + t inside a row; records the call."""

    def __init__(self, hop):
        self.hop, self.calls = hop, []

    def __call__(self, units, f0, volume, spk_id, spk_mix_dict=None, n_frames=None, **kw):
        self.calls.append(dict(units=units, f0=f0, volume=volume, spk_id=spk_id, n_frames=list(n_frames), kw=kw))
        B, Fr = units.shape[0], units.shape[1]
        t = torch.arange(Fr * self.hop)
        sig = 1000.0 * units[:, :, 0].repeat_interleave(self.hop, dim=1) + t[None, :].float()
        return sig, None, (sig, sig)


def test_ragged_plan_render_local_with_a_stub_model():
    from sharding import RaggedPlan
    hop = 4
    n_frames = [5, 2, 9, 1, 7, 3]
    plan = RaggedPlan(n_frames, world=2, hop=hop)
    units = [torch.full((n, 3), float(i + 1)) for i, n in enumerate(n_frames)]
    f0 = [torch.full((1, n, 1), 100.0 + i) for i, n in enumerate(n_frames)]       # a leading batch dimension is accepted
    volume = [torch.full((n,), 0.1 * i) for i, n in enumerate(n_frames)]
    spk = torch.arange(1, 7).reshape(6, 1)
    flats = []
    for rank in range(2):
        stub = _StubModel(hop)
        rendered = plan.render_local(stub, rank, units, f0, volume, spk, noise_seed=5)
        idx = plan.local(rank)
        assert len(stub.calls) == 1 and len(rendered) == len(idx)                      # ONE forward per rank
        call = stub.calls[0]
        assert call["n_frames"] == [n_frames[i] for i in idx] and call["kw"] == {"noise_seed": 5}
        assert call["units"].shape == (len(idx), max(n_frames[i] for i in idx), 3)
        assert call["f0"].shape[2] == 1 and call["volume"].dim() == 2
        assert call["spk_id"].reshape(-1).tolist() == [i + 1 for i in idx]
        for j, i in enumerate(idx):
            assert float(call["units"][j, n_frames[i]:].abs().sum()) == 0.0          # zero padding
            assert float(call["f0"][j, 0, 0]) == 100.0 + i
            want = 1000.0 * (i + 1) + torch.arange(n_frames[i] * hop).float()
            assert torch.equal(rendered[j], want)
        flats.append(plan.pack(rank, rendered))
    out = plan.unpack(torch.cat(flats))
    for i, n in enumerate(n_frames):
        assert torch.equal(out[i], 1000.0 * (i + 1) + torch.arange(n * hop).float())
    # a rank without work renders nothing; a broadcast speaker id is passed through
    plan1 = RaggedPlan([4], world=2, hop=hop)
    assert plan1.render_local(_StubModel(hop), 1, [units[0][:4]], [f0[0][:, :4]], [volume[0][:4]], spk[:1]) == []
    stub = _StubModel(hop)
    plan.render_local(stub, 0, units, f0, volume, spk[:1])
    assert stub.calls[0]["spk_id"].shape == (1, 1)
