"""The silence slicer on the device: `ddsp_slicer` behind `slicer.Slicer` and `infer_offline.split`.

Yardsticks: tests/golden/slicer_ref.npz - the chunks the reference's own `Slicer.slice` returned on the seeded signals of
tests/slicer_cases.py, under both pad modes (tests/golden/make_golden_slicer.py) - compared exactly: the cases keep every
frame's RMS more than 1e-3 (relative) off the threshold and every evaluated argmin's minimum either tied exactly or more than
1e-3 below its runner-up (`slicer_cases.check_conditions`), so fp32 summation order cannot change a decision.  The frame RMS
itself is compared with the fp64 restatement of librosa's documented definition; the gate is `slicer_cases.RMS_RTOL` = 4.3e-7,
four times the largest relative difference of the fp32 restatement from the fp64 one on these cases (measured: 1.07e-7).
Outputs are prefilled (-7 / NaN), so a cell the kernels did not write shows."""
import os

import numpy as np
import pytest
import torch

import slicer_cases as SC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASE_MODES = [(name, mode) for name in SC.CASES for mode in SC.PAD_MODES]


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "slicer_ref.npz"))


@pytest.fixture(scope="module")
def rms64():
    """{(case, pad mode): the fp64 restatement's frame RMS} - computed once."""
    return {(name, mode): SC.restate(name, mode, np.float64)[2] for name, mode in CASE_MODES}


def _slicer(name, mode, dev):
    from slicer import Slicer
    return Slicer(**SC.PARAMS[SC.CASES[name][0]], pad_mode=mode, device=dev)


def _prefilled(ctx, s, B, T, dev, capacity=None):
    import hipddsp
    F = s.frames(T)
    cap = hipddsp.slicer_capacity(F, s.min_interval) if capacity is None else capacity
    return (torch.full((B, cap, 3), -7, device=dev, dtype=torch.int32), torch.full((B,), -7, device=dev, dtype=torch.int32),
            torch.full((B, F), float("nan"), device=dev))


def _run(ctx, s, x, dev, n_dev=None, capacity=None):
    out = _prefilled(ctx, s, x.shape[0], x.shape[1], dev, capacity)
    return ctx.slicer(x, s.win_size, s.hop_size, s.threshold, s.min_length, s.min_interval, s.max_sil_kept, pad_mode=s.pad_mode,
                      n_dev=n_dev, capacity=capacity, out=out)


@pytest.fixture(scope="module")
def solo(ctx, dev):
    """{(case, pad mode): (table, count, rms) on the host of the case cut alone} - computed once."""
    out = {}
    for name, mode in CASE_MODES:
        x = torch.from_numpy(SC.signal(name)).to(dev)[None]
        table, count, rms = _run(ctx, _slicer(name, mode, dev), x, dev)
        out[name, mode] = (table[0].cpu().numpy(), int(count[0]), rms[0].cpu().numpy())
    ctx.poll_error()
    return out


def test_rms_against_the_fp64_restatement(solo, rms64):
    worst = 0.0
    for key, (_, _, rms) in solo.items():
        d = SC.rms_difference(rms, rms64[key])
        print(f"{key[0]:9s} {key[1]:8s} frame RMS against the fp64 restatement: {d:.3e}")
        worst = max(worst, d)
    assert worst <= SC.RMS_RTOL, worst


@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_chunks_equal_the_reference_solo(g, solo, name, mode):
    table, count, _ = solo[name, mode]
    want = g[f"{name}_{mode}_chunks"]
    assert count == want.shape[0], (count, want.shape[0])
    assert np.array_equal(table[:count], want)
    assert not table[count:].any()                       # rows from the count on are zeros


@pytest.mark.parametrize("mode", SC.PAD_MODES)
def test_ragged_batches_equal_the_solo_rows(ctx, dev, solo, mode):
    """The cases of one parameter set as one ragged batch (B <= 8), the padding behind every row filled with loud values and
    NaN: every row equals its solo result bit for bit, the frames behind a row's own are 0."""
    import hipddsp
    batches = 0
    for pset in SC.PARAMS:
        names = [n for n in SC.CASES if SC.CASES[n][0] == pset]
        for k in range(0, len(names), 8):
            group = names[k:k + 8]
            sigs = [SC.signal(n) for n in group]
            T = max(x.shape[0] for x in sigs) + 7
            x = torch.empty(len(group), T)
            x[:, 0::2], x[:, 1::2] = 0.9, float("nan")
            for b, v in enumerate(sigs):
                x[b, :v.shape[0]] = torch.from_numpy(v)
            s = _slicer(group[0], mode, dev)
            counts = hipddsp.check_n_samples([v.shape[0] for v in sigs], len(group), T, hipddsp.slicer_rule)
            table, count, rms = _run(ctx, s, x.to(dev), dev, n_dev=ctx.ragged_counts(counts))
            table, count, rms = table.cpu().numpy(), count.cpu().numpy(), rms.cpu().numpy()
            for b, name in enumerate(group):
                want_table, want_count, want_rms = solo[name, mode]
                F = want_rms.shape[0]
                assert count[b] == want_count, (name, count[b], want_count)
                assert np.array_equal(table[b, :want_count], want_table[:want_count]), name
                assert not table[b, want_count:].any(), name
                assert np.array_equal(rms[b, :F], want_rms) and not rms[b, F:].any(), name      # (NaN != 0: none leaked)
            batches += 1
    ctx.poll_error()
    assert batches >= len(SC.PARAMS)


def test_chunks_takes_a_ragged_batch(dev, solo):
    names = [n for n in SC.CASES if SC.CASES[n][0] == "base"][:4]
    sigs = [SC.signal(n) for n in names]
    x = np.full((len(names), max(v.shape[0] for v in sigs)), 0.5, dtype=np.float32)
    for b, v in enumerate(sigs):
        x[b, :v.shape[0]] = v
    table, count, rms = _slicer(names[0], "constant", dev).chunks(x, n_samples=[v.shape[0] for v in sigs])
    assert table.is_cuda and count.is_cuda and rms.is_cuda and table.dtype == count.dtype == torch.int32
    for b, name in enumerate(names):
        want_table, want_count, _ = solo[name, "constant"]
        assert int(count[b]) == want_count and np.array_equal(table[b, :want_count].cpu().numpy(), want_table[:want_count])
    with pytest.raises(ValueError, match=r"n_samples\[1\] = 0"):
        _slicer(names[0], "constant", dev).chunks(x, n_samples=[5, 0, 5, 5])


@pytest.mark.parametrize("name,mode", [("all_a", "constant"), ("all_b", "reflect"), ("zeros", "constant"), ("early", "constant"),
                                       ("odd_b", "reflect")])
def test_slice_returns_the_reference_dict(g, dev, name, mode):
    want = SC.chunk_dict(g[f"{name}_{mode}_chunks"])
    s = _slicer(name, mode, dev)
    assert s.slice(SC.signal(name)) == want                                       # numpy in
    assert s.slice(torch.from_numpy(SC.signal(name)).to(dev)) == want             # a device tensor in


def test_cut_is_the_reference_cut(dev):
    from slicer import Slicer, cut
    x = SC.signal("split_a")
    got = cut(x, SC.SR, db_thresh=-40, min_len=300)
    assert got == Slicer(SC.SR, threshold=-40, min_length=300).slice(x) and len(got) == 4


def test_a_small_capacity_sets_the_error_word(ctx, dev, g):
    """A table of 3 rows for a row of 9 chunks: the chunks that fit are written, the count is the capacity, nothing is written
    behind the table, and the context reports it - an error code, not a fault."""
    want = g["all_a_constant_chunks"]
    assert want.shape[0] > 3
    s = _slicer("all_a", "constant", dev)
    x = torch.from_numpy(SC.signal("all_a")).to(dev)[None]
    guard = torch.full((2, 3, 3), -7, device=dev, dtype=torch.int32)          # row 1 stands behind the table of row 0
    out = (guard[:1], torch.full((1,), -7, device=dev, dtype=torch.int32), torch.empty(1, s.frames(x.shape[1]), device=dev))
    table, count, _ = ctx.slicer(x, s.win_size, s.hop_size, s.threshold, s.min_length, s.min_interval, s.max_sil_kept,
                                 capacity=3, out=out)
    torch.cuda.synchronize()
    assert int(count[0]) == 3 and np.array_equal(table[0].cpu().numpy(), want[:3])
    assert bool((guard[1] == -7).all())
    with pytest.raises(ValueError, match="capacity"):
        ctx.poll_error()
    ctx.poll_error()                                                            # reported once, then clear


def test_split_on_the_fixture_case(g, dev):
    import infer_offline
    rows = g["split_a_constant_chunks"]
    want = [(int(a), int(b)) for a, b, _ in rows if a != b]
    assert infer_offline.split(SC.signal("split_a"), SC.SR, 160.0, db_thresh=-40, min_len=300) == want and len(want) == 2
    assert infer_offline.split(torch.from_numpy(SC.signal("split_a")).to(dev), SC.SR, 160.0, -40, 300) == want


# ---- infer_offline.convert(..., slices=None, ...) ---------------------------------------------------------------------------
SR, HOP = 44100, 512


def _speech_and_silence():
    """3 s at 44.1 kHz: 2 s of a harmonic tone, then 1 s of noise floor that is quietest from 2.3 to 2.5 s - with main.py's
    defaults (5 s minimum length) the slicer tags the trailing silence at its quietest frame, so `split` returns a voiced range
    and a silence range."""
    rng = np.random.default_rng(41)
    t = np.arange(2 * SR) / SR
    voiced = 0.3 * np.sin(2 * np.pi * 190.7 * t) + 0.1 * np.sin(2 * np.pi * 381.4 * t + 0.3) + 1e-3 * rng.standard_normal(len(t))
    floor = 1e-4 * rng.standard_normal(SR)
    floor[int(0.3 * SR):int(0.5 * SR)] *= 0.1
    return np.concatenate([voiced, floor]).astype(np.float32)


def test_convert_without_slices_is_convert_with_split(dev, lib_path, tmp_path):
    import hubert_cases as HC
    import infer_offline
    import synthetic
    from ddsp.hubert import HubertSoft
    from ddsp.vocoder import DotDict, F0_Extractor, Units_Encoder
    path = str(tmp_path / "hubert-soft.pt")
    torch.save(HC.fill({k: tuple(v.shape) for k, v in HubertSoft().state_dict().items()}), path)
    encoder = Units_Encoder("hubertsoft", path, device=dev)
    extractor = F0_Extractor("ac", SR, HOP, 65.0, 800.0, device=dev)
    model, _ = synthetic.build_model("CombSub", seed=8, device=dev)
    args = DotDict({"data": {"block_size": HOP, "sampling_rate": SR}})
    spk = torch.full((1, 1), 2, dtype=torch.int64, device=dev)
    audio = _speech_and_silence()
    slices = infer_offline.split(audio, SR, float(HOP))
    assert len(slices) == 2 and slices[0][0] == 0 and slices[0][1] == slices[1][0] and slices[1][1] == audio.shape[0]
    assert int(2.3 * SR) <= slices[0][1] <= int(2.5 * SR) and slices[0][1] % 882 == 0      # the cut lies in the quietest part
    got, sr_g = infer_offline.convert(model, args, audio, SR, None, encoder, extractor, spk, noise_seed=5)
    want, sr_w = infer_offline.convert(model, args, audio, SR, slices, encoder, extractor, spk, noise_seed=5)
    assert sr_g == sr_w == SR and got.dtype == np.float64 and got.shape == want.shape and got.shape[0] > 2 * SR
    assert np.array_equal(got, want) and float(np.abs(got).max()) > 1e-3
