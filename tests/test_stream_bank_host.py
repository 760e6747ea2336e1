"""Host side of the stream bank: the refusals of `hipddsp.check_mix_rows`, the `spk_mix_rows` / `spk_mix_dict` exclusion of the
synthesisers (raised before anything needs a device) and `realtime.bank_sizes` against the helpers `StreamRenderer` uses."""
import pytest
import torch

import synthetic


def _tables(B=3, K=3):
    return torch.ones(B, K, dtype=torch.int32), torch.zeros(B, K, dtype=torch.float32)


def test_check_mix_rows_refusals(lib_path):
    import hipddsp
    ids, w = _tables()
    assert hipddsp.check_mix_rows(ids, w, 3, 100) == 3
    assert hipddsp.check_mix_rows(*_tables(2, 16), 2, 100) == 16
    bad = [
        (ids.long(), w, 3),                       # ids must be int32
        (ids, w.double(), 3),                     # weights must be fp32
        (ids, w, 4),                              # another batch
        (ids[:, :2], w, 3),                       # shapes differ
        (ids[0], w[0], 3),                        # not 2-D
        (*_tables(3, 17), 3),                     # K > 16
        (*_tables(3, 0), 3),                      # K = 0
        (ids.t().contiguous().t(), w, 3),         # not contiguous
        (ids.tolist(), w, 3),                     # not tensors
    ]
    for i, ww, B in bad:
        with pytest.raises(ValueError):
            hipddsp.check_mix_rows(i, ww, B, 100)
    for v in (0, 101, -1):                        # ids of host tables are checked against n_spk
        j = ids.clone()
        j[1, 2] = v
        with pytest.raises(ValueError):
            hipddsp.check_mix_rows(j, w, 3, 100)


def test_mix_rows_builds_padded_tables(lib_path):
    import hipddsp
    ids, w = hipddsp.mix_rows([2, {1: 0.3, 5: 0.7}, {7: 0.5, 3: 0.25, 4: 0.25}], 3, 100)
    assert ids.tolist() == [[2, 1, 1], [1, 5, 1], [7, 3, 4]] and ids.dtype == torch.int32
    assert torch.equal(w, torch.tensor([[1.0, 0, 0], [0.3, 0.7, 0], [0.5, 0.25, 0.25]]))
    for bad in ([{}], [{1: 1.0, 2: 1.0, 3: 1.0, 4: 1.0}], [101], [0]):
        with pytest.raises(ValueError):
            hipddsp.mix_rows(bad, 3, 100)


@pytest.mark.parametrize("name", ["CombSub", "Sins", "CombSubFast"])
def test_mix_rows_exclusion_and_grad_mode(lib_path, name):
    model, _ = synthetic.build_model(name, seed=3)
    inp = synthetic.make_inputs(4, 3, 5)
    ids, w = _tables()
    args = (inp["units"], inp["f0"], inp["volume"], inp["spk_id"])
    with torch.no_grad():
        with pytest.raises(ValueError):
            model(*args, spk_mix_dict={1: 1.0}, spk_mix_rows=(ids, w))
        with pytest.raises(ValueError):
            model(*args, spk_mix_rows=(ids[:2], w[:2]))
        with pytest.raises(ValueError):
            model(*args, spk_mix_rows=ids)
    with pytest.raises(NotImplementedError):      # grad mode on, parameters want gradients
        model(*args, spk_mix_rows=(ids, w))
    with torch.no_grad(), pytest.raises(RuntimeError):   # well-formed tables reach the device check: no CPU fallback
        model(*args, spk_mix_rows=(ids, w))


@pytest.mark.parametrize("sr", [44100, 48000])
@pytest.mark.parametrize("timing", [(0.2, 0.04, 4), (1.5, 0.03, 2)], ids=["config5", "gui"])
def test_bank_sizes_against_renderer_helpers(sr, timing):
    import realtime
    block_time, xfade_time, buffer_num = timing
    z = realtime.bank_sizes(sr, block_time, xfade_time, buffer_num, 512, 44100)
    assert z["n_in"] == realtime.input_frames(sr, block_time, xfade_time, buffer_num)
    assert z["hop_size"] == realtime.hop_size(512, sr, 44100)
    assert z["frames"] == realtime.window_frames(z["n_in"], z["hop_size"])
    assert z["silence_front"] == realtime.silence_front(block_time, buffer_num, xfade_time)
    assert (z["block"], z["xfade"], z["search"], z["delay"]) == (int(block_time * sr), int(xfade_time * sr), int(0.01 * sr), int(0.02 * sr))
    if sr == 44100:
        assert z["frames"] == (87 if block_time == 0.2 else 388)
