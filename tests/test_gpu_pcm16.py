"""`ddsp_pcm16` (`Context.pcm16`, `infer_offline.to_pcm16`): the 16-bit PCM of a stitched fp64 waveform on the device against
the host statement `main.pcm16` (numpy's `clip(rint(x * 32768), -32768, 32767).astype(int16)`), sample for sample, with the
spans' peak and clipped counts.  Everything is exact: the kernel rounds half to even as numpy's rint does, the product by 2^15 is
exact, and a maximum of |x| and a count have no rounding.

The input: 4099 samples - no multiple of 4 - viewed from element 1 of a larger tensor, so its base is 8-byte but not 16-byte
aligned (the word path), and the same values from element 0 (the 16-byte path).  It holds every tie (k + 0.5) / 32768 for k in
-4..4, +-1.0, +-(1 - 2^-16), +-1.5, +-1e9, +-0.0, denormals, and U(-1.2, 1.2) elsewhere.  NaN is out of contract."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N = 4099
SPANS = [(0, 1025), (1026, 1500), (3000, 1099)]          # an odd span, then the 1-sample rounding gap; a gap of 474; the end


def _wave():
    rng = np.random.Generator(np.random.PCG64(1616))
    x = rng.uniform(-1.2, 1.2, N)
    special = [(k + 0.5) / 32768 for k in range(-4, 5)] + [1.0, -1.0, 1 - 2.0 ** -16, -(1 - 2.0 ** -16), 1.5, -1.5, 1e9, -1e9,
                                                           0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1030, -(2.0 ** -1040)]
    # spread over the three spans, a few at the spans' edges and in both gaps
    at = [0, 1, 2, 3, 5, 1023, 1024, 1025, 1026, 1027, 1030, 2000, 2524, 2525, 2526, 3500, 4095, 3000, 3001, 2700, 2999, 4096, 4097,
          4098, 700, 701, 1500, 3333]
    for i, v in zip(at, special + special[:len(at) - len(special)]):
        x[i] = v
    return x


def _stats(x, spans):
    r = np.rint(x * 32768.0)
    return ([float(np.abs(x[b:b + n]).max()) if n else 0.0 for b, n in spans],
            [int(((r[b:b + n] < -32768) | (r[b:b + n] > 32767)).sum()) for b, n in spans])


@pytest.mark.parametrize("offset", [1, 0])
def test_pcm16_equals_the_host_statement(ctx, dev, lib_path, offset):
    import infer_offline
    import main
    x = _wave()
    buf = torch.zeros(N + 2, dtype=torch.float64)
    buf[offset:offset + N] = torch.from_numpy(x)
    wave = buf.to(dev)[offset:offset + N]
    assert (wave.data_ptr() % 16 == 8) == (offset == 1) and wave.is_contiguous()
    want = main.pcm16(x)
    ties = [int(v) for v in main.pcm16([(k + 0.5) / 32768 for k in range(-4, 5)])]
    assert ties == [-4, -2, -2, 0, 0, 2, 2, 4, 4] and {-32768, 32767} <= set(want.tolist())   # half to even, both ways
    covered = np.zeros(N, dtype=bool)
    for b, n in SPANS:
        covered[b:b + n] = True
    assert int((~covered).sum()) == 1 + 474
    got, peak, clipped = ctx.pcm16(wave, SPANS)
    assert got.dtype == torch.int16 and got.shape == (N,) and peak.dtype == torch.float64 and clipped.dtype == torch.int64
    host = got.cpu().numpy()
    assert np.array_equal(host[covered], want[covered])
    assert not host[~covered].any() and want[~covered].any()                            # the gaps are 0 whatever x holds there
    want_peak, want_clipped = _stats(x, SPANS)
    print("peak", peak.tolist(), "clipped", clipped.tolist())
    assert peak.tolist() == want_peak and clipped.tolist() == want_clipped
    assert min(want_clipped) > 0 and want_peak[2] == 1e9
    # no spans: one span over everything
    got, peak, clipped = ctx.pcm16(wave)
    want_peak, want_clipped = _stats(x, [(0, N)])
    assert np.array_equal(got.cpu().numpy(), want) and peak.tolist() == want_peak and clipped.tolist() == want_clipped
    # the module's entry, and the lengths around a workgroup's tile and a thread's four samples
    again = infer_offline.to_pcm16(wave, SPANS)
    assert torch.equal(again[0], torch.from_numpy(np.where(covered, want, 0).astype(np.int16)).to(dev))
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 2049):
        got, peak, clipped = ctx.pcm16(wave[:n])
        assert np.array_equal(got.cpu().numpy(), want[:n]) and peak.tolist() == _stats(x[:n], [(0, n)])[0], n
    torch.cuda.synchronize()
    ctx.poll_error()


def test_pcm16_of_nothing_and_bad_spans(ctx, dev, lib_path):
    wave = torch.from_numpy(_wave()).to(dev)
    got, peak, clipped = ctx.pcm16(wave[:0])
    assert got.numel() == 0 and peak.tolist() == [0.0] and clipped.tolist() == [0]
    got, peak, clipped = ctx.pcm16(wave, [])
    assert not got.any() and got.shape == (N,) and peak.numel() == 0 and clipped.numel() == 0
    got, peak, clipped = ctx.pcm16(wave, [(0, 0), (0, 8), (8, 0)])                      # empty spans (a file without slices)
    assert peak.tolist() == _stats(_wave(), [(0, 0), (0, 8), (8, 0)])[0] and not got[8:].any() and clipped.tolist()[0] == 0
    for spans in ([(1, 10)], [(0, 10), (8, 4)], [(0, N + 1)], [(4, -1)]):
        with pytest.raises(ValueError, match="pcm16: span"):
            ctx.pcm16(wave, spans)
    with pytest.raises(ValueError, match="fp64"):
        ctx.pcm16(wave.float())
