"""The envelope mix on the device: `ddsp_envelope_rms` and `ddsp_envelope_apply` against their numpy statement
(tests/envelope_cases.py, RVC's `change_rms`), offline jobs with an envelope, and `StreamBank(envelope=True)`.

Bounds, derived and not measured.  A frame's sum of at most 2^17 fp64 terms in another order differs by at most
2^17 * 2^-53 = 1.5e-11 relative; sqrt, two pow and the interpolation add a few ulp.  The gate is `EC.ENV_GATE` = 1e-10 relative
on the envelopes and 1e-10 relative plus 1e-300 absolute on an fp64 output.  An fp32 output is the fp64 product rounded once
more: where that product lies within 1e-10 of a rounding boundary the two roundings differ by one fp32 ulp, so the fp32 form
is held to 1e-10 relative plus one ulp of fp32 (2^-23 relative).  Rows with rate == 1, rows without an owner, refused rows and
every element outside the spans or behind a count: their bits.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import envelope_cases as EC
from test_gpu_many import encoder  # noqa: F401  (the module-scoped random-weight HubertSoft fixture)
from test_gpu_many_jobs import extractor  # noqa: F401

pytestmark = pytest.mark.gpu


def _i32(dev, a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev)


def _i64(dev, a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int64).to(dev)


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _matrix(rows, T, dtype=np.float32):
    """Ragged rows -> (R, T) with NaN behind every count."""
    x = np.full((len(rows), T), np.nan, dtype=dtype)
    for r, row in enumerate(rows):
        x[r, :len(row)] = row
    return x


def _spans(rows, bases, total):
    """fp64 rows at `bases` of a NaN-filled tensor -> (tensor, [(base, count)])."""
    x = np.full(total, np.nan, dtype=np.float64)
    for row, base in zip(rows, bases):
        x[base:base + len(row)] = row
    return x, [(int(b), len(row)) for row, b in zip(rows, bases)]


def _hold_env(got, rows, hop, m, what):
    """env (R, N_max) of the device against the statement of every row: finite, 0 behind the row's frames, within the gate."""
    assert np.isfinite(got).all()
    worst = 0.0
    for r, row in enumerate(rows):
        want = EC.frame_rms(row, hop, m)
        assert got.shape[1] >= len(want) and not got[r, len(want):].any()
        worst = max(worst, EC.rel_err(got[r, :len(want)], want))
    print(f"{what}: {len(rows)} rows, envelope off by at most {worst:.3e} relative (gate {EC.ENV_GATE:g})")
    assert worst <= EC.ENV_GATE


# ---- 1. frame RMS ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,m", EC.RMS_SETTINGS)
def test_rms_matches_the_statement_at_every_length(ctx, dev, hop, m):
    ctx.poll_error()
    for n in EC.rms_lengths(hop):
        row = EC.signal(n, seed=n)
        x = _matrix([row], n + 3)
        got = ctx.envelope_rms(_t(dev, x), hop, m, n_samples=_i32(dev, [n]))
        assert tuple(got.shape) == (1, 1 + (n + 3) // hop) and got.dtype == torch.float64
        _hold_env(got.cpu().numpy(), [row], hop, m, f"hop {hop}, m {m}, n {n}")
    torch.cuda.synchronize()
    ctx.poll_error()


@pytest.mark.parametrize("hop,m", EC.RMS_SETTINGS)
def test_rms_of_a_ragged_batch_and_of_spans_at_odd_bases(ctx, dev, hop, m):
    ctx.poll_error()
    lengths = (37, 1, 2 * hop + 3, hop)
    rows = [EC.signal(n, seed=10 + k) for k, n in enumerate(lengths)]
    x = _matrix(rows, 39)                                                # (T_max is no multiple of 4: rows start at odd alignments)
    a = ctx.envelope_rms(_t(dev, x), hop, m, n_samples=_i32(dev, lengths))
    b = ctx.envelope_rms(_t(dev, x), hop, m, n_samples=_i32(dev, lengths))
    _hold_env(a.cpu().numpy(), rows, hop, m, f"ragged batch, hop {hop}, m {m}")
    assert EC.same_bits(a.cpu().numpy(), b.cpu().numpy())               # the same input gives the same bits
    rows64 = [EC.signal(n, seed=20 + k, dtype=np.float64) for k, n in enumerate(lengths)]
    y, spans = _spans(rows64, (1, 41, 43, 43 + 2 * hop + 3 + 2), 120)    # odd bases: every 16-byte load starts off the row's start
    got = ctx.envelope_rms(_t(dev, y), hop, m, spans=_i64(dev, spans), n_max=max(lengths))
    _hold_env(got.cpu().numpy(), rows64, hop, m, f"spans, hop {hop}, m {m}")
    torch.cuda.synchronize()
    ctx.poll_error()


@pytest.mark.parametrize("hop,m,n", [EC.OFFLINE, EC.LIVE], ids=["offline", "live"])
def test_rms_at_the_offline_and_the_live_size(ctx, dev, hop, m, n):
    ctx.poll_error()
    row = EC.signal(n, seed=3)
    x = _matrix([row], n + 2)
    got = ctx.envelope_rms(_t(dev, x), hop, m, n_samples=_i32(dev, [n]))
    again = ctx.envelope_rms(_t(dev, x), hop, m, n_samples=_i32(dev, [n]))
    _hold_env(got.cpu().numpy(), [row], hop, m, f"hop {hop}, m {m}, n {n}")
    assert EC.same_bits(got.cpu().numpy(), again.cpu().numpy())
    row64 = EC.signal(n, seed=4, dtype=np.float64)
    y, spans = _spans([row64], (3,), n + 8)
    got = ctx.envelope_rms(_t(dev, y), hop, m, spans=_i64(dev, spans), n_max=n)
    _hold_env(got.cpu().numpy(), [row64], hop, m, f"span, hop {hop}, m {m}, n {n}")
    torch.cuda.synchronize()
    ctx.poll_error()


# ---- 2. the apply ---------------------------------------------------------------------------------------------------------------
HOP1, HOP2, M = 4, 11, 2
RATES = (0.25, 0.0, 1.0, 0.5)


def _apply_case(dtype):
    """Sources (fp32, ragged) and output rows of `dtype` with (source, owner) per row; owner -1: a row without the control."""
    sources = [EC.signal(37, seed=1), np.zeros(37, dtype=np.float32), EC.signal(3, seed=2)]      # row 1: exact zeros; row 2: N1 = 1
    outs = [EC.signal(101, seed=30 + k, dtype=dtype) for k in range(4)]
    outs.append(EC.signal(101, seed=40, scale=1e-9, dtype=dtype))        # below the floor: e2 = 1e-6 everywhere
    outs.append(EC.signal(7, seed=41, dtype=dtype))                      # N2 = 1: a constant envelope
    outs.append(EC.signal(101, seed=42, dtype=dtype))
    src_of_row = [0, 0, 0, 1, 0, 2, 0]
    owner = [0, 1, 2, 0, 0, 3, -1]                                       # rates 0.25, 0, 1, 0.25, 0.25, 0.5, none
    return sources, outs, src_of_row, owner


def _want(sources, outs, src_of_row, owner, rates):
    return [o.copy() if j < 0 or j >= len(rates) else EC.mix(sources[s], HOP1, o, HOP2, M, rates[j])
            for o, s, j in zip(outs, src_of_row, owner)]


def _device_apply(ctx, dev, sources, outs, src_of_row, owner, rates, fp32, spans_for_apply=None):
    """RMS of the sources, RMS of the outputs, the apply -> (the whole output array after the call, before it, the row slices)."""
    lengths = [len(s) for s in sources]
    src = ctx.envelope_rms(_t(dev, _matrix(sources, max(lengths) + 2)), HOP1, M, n_samples=_i32(dev, lengths))
    n_out = [len(o) for o in outs]
    kw = dict(src_of_row=_i32(dev, src_of_row), owner=None if owner is None else _i32(dev, owner))
    if fp32:
        before = _matrix(outs, max(n_out) + 3)
        y = _t(dev, before)
        env = ctx.envelope_rms(y, HOP2, M, n_samples=_i32(dev, n_out))
        got = ctx.envelope_mix_(y, src, _t(dev, np.asarray(rates, dtype=np.float64)), env, HOP2, HOP1, _i32(dev, lengths),
                                n_out=_i32(dev, n_out), **kw)
        where = [(r, slice(0, n)) for r, n in enumerate(n_out)]
    else:
        bases, at = [], 1
        for n in n_out:
            bases.append(at)
            at += n + 3                                                  # gaps between the spans, odd and even bases
        before, spans = _spans(outs, bases, at + 5)
        y = _t(dev, before)
        env = ctx.envelope_rms(y, HOP2, M, spans=_i64(dev, spans), n_max=max(n_out))
        got = ctx.envelope_mix_(y, src, _t(dev, np.asarray(rates, dtype=np.float64)), env, HOP2, HOP1, _i32(dev, lengths),
                                spans=_i64(dev, spans if spans_for_apply is None else spans_for_apply(spans, before.size)),
                                n_max=max(n_out), **kw)
        where = [slice(b, b + n) for b, n in spans]
    assert got is y
    torch.cuda.synchronize()
    return got.cpu().numpy(), before, where


def _hold_rows(got, before, where, want, outs, keep, fp32, what):
    """Every row against the statement at the gate; rows in `keep` and every element outside the rows keep their bits."""
    outside = np.ones(before.shape, dtype=bool)
    worst = 0.0
    for r, (w, o) in enumerate(zip(want, outs)):
        outside[where[r]] = False
        g = got[where[r]]
        if r in keep:
            assert EC.same_bits(g, o), f"{what}: row {r} must keep its bits"
            continue
        assert np.isfinite(g).all()
        w64, g64 = w.astype(np.float64), g.astype(np.float64)
        slack = np.abs(w64) * 2.0 ** -23 if fp32 else 1e-300
        excess = np.abs(g64 - w64) - (EC.ENV_GATE * np.abs(w64) + slack)
        nz = w64 != 0
        worst = max(worst, float(np.max(np.abs(g64 - w64)[nz] / np.abs(w64)[nz])) if nz.any() else 0.0)
        assert (excess <= 0).all(), f"{what}: row {r} off by {worst:.3e} relative"
    print(f"{what}: output off by at most {worst:.3e} relative (gate {EC.ENV_GATE:g}" + (" + one fp32 ulp)" if fp32 else ")"))
    assert EC.same_bits(got[outside], before[outside]), f"{what}: an element outside the rows was written"


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64-spans", "fp32-matrix"])
def test_apply_matches_the_statement(ctx, dev, fp32):
    ctx.poll_error()
    sources, outs, src_of_row, owner = _apply_case(np.float32 if fp32 else np.float64)
    want = _want(sources, outs, src_of_row, owner, RATES)
    got, before, where = _device_apply(ctx, dev, sources, outs, src_of_row, owner, RATES, fp32)
    _hold_rows(got, before, where, want, outs, keep={2, 6}, fp32=fp32, what="apply")
    assert not got[where[3]].any() and not want[3].any()                 # a silent source: the gain is exactly 0
    e2 = EC.interpolate(EC.frame_rms(outs[4], HOP2, M), len(outs[4]))
    assert (e2 < EC.FLOOR).all()                                         # row 4 takes the 1e-6 branch at every sample
    again, _, _ = _device_apply(ctx, dev, sources, outs, src_of_row, owner, RATES, fp32)
    assert EC.same_bits(got, again)                                      # two runs, identical bits
    ctx.poll_error()


def test_apply_without_owner_and_source_tables(ctx, dev):
    """owner=None, src_of_row=None: row r takes rate r and source r; the sources' count as one host int."""
    ctx.poll_error()
    sources = [EC.signal(37, seed=50 + k) for k in range(3)]
    outs = [EC.signal(101, seed=60 + k, dtype=np.float64) for k in range(3)]
    rates = (0.0, 1.0, 0.25)
    src = ctx.envelope_rms(_t(dev, _matrix(sources, 37)), HOP1, M)
    before, spans = _spans(outs, (0, 102, 205), 310)
    y = _t(dev, before)
    env = ctx.envelope_rms(y, HOP2, M, spans=_i64(dev, spans), n_max=101)
    ctx.envelope_mix_(y, src, _t(dev, np.asarray(rates)), env, HOP2, HOP1, 37, spans=_i64(dev, spans), n_max=101)
    torch.cuda.synchronize()
    want = [EC.mix(s, HOP1, o, HOP2, M, r) for s, o, r in zip(sources, outs, rates)]
    _hold_rows(y.cpu().numpy(), before, [slice(b, b + n) for b, n in spans], want, outs, keep={1}, fp32=False, what="plain rows")
    ctx.poll_error()


# ---- 3. refusals on the device: the error word, not a fault ----------------------------------------------------------------------
def _bad_span(spans, total):
    return [spans[0], (total - 50, 101)] + spans[2:]                     # row 1 would end 51 elements behind the tensor


@pytest.mark.parametrize("what", ["rate 1.5", "rate NaN", "owner J", "span"])
def test_a_refused_row_keeps_its_bits_and_raises_the_error_word(ctx, dev, what):
    ctx.poll_error()
    sources, outs, src_of_row, owner = _apply_case(np.float64)
    rates, owner, kw = list(RATES), list(owner), {}
    if what == "rate 1.5":
        rates[1] = 1.5
    elif what == "rate NaN":
        rates[1] = float("nan")
    elif what == "owner J":
        owner[1] = len(rates)
    else:
        kw["spans_for_apply"] = _bad_span
    want = _want(sources, outs, src_of_row, owner, rates)                # (row 1 keeps its bits in the statement too)
    got, before, where = _device_apply(ctx, dev, sources, outs, src_of_row, owner, rates, False, **kw)
    with pytest.raises(ValueError, match="envelope"):
        ctx.poll_error()
    ctx.poll_error()                                                     # taken: the word is clear again
    _hold_rows(got, before, where, want, outs, keep={1, 2, 6}, fp32=False, what=f"refused ({what})")


def test_rms_refuses_a_span_that_leaves_the_tensor(ctx, dev):
    ctx.poll_error()
    rows = [EC.signal(37, seed=70 + k, dtype=np.float64) for k in range(2)]
    y, spans = _spans(rows, (1, 41), 80)
    got = ctx.envelope_rms(_t(dev, y), 4, 2, spans=_i64(dev, [spans[0], (60, 37)]), n_max=37)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="envelope"):
        ctx.poll_error()
    got = got.cpu().numpy()
    _hold_env(got[:1], rows[:1], 4, 2, "the row beside a refused span")
    assert not got[1].any()


def test_the_binding_refuses_before_the_launch(ctx, dev):
    x = torch.zeros(2, 16, device=dev)
    y = torch.zeros(40, dtype=torch.float64, device=dev)
    spans = _i64(dev, [(0, 16), (20, 16)])
    for bad in (dict(m=3), dict(m=10), dict(hop=0), dict(hop=2.0), dict(n_samples=torch.zeros(2, dtype=torch.int32)),
                dict(n_samples=_i32(dev, [1, 2, 3])), dict(spans=spans)):
        with pytest.raises(ValueError):
            ctx.envelope_rms(x, **{"hop": 4, **bad})
    for bad in (dict(), dict(spans=spans), dict(spans=spans, n_max=0), dict(spans=spans.int(), n_max=16),
                dict(spans=spans, n_max=16, n_samples=_i32(dev, [16, 16]))):
        with pytest.raises(ValueError):
            ctx.envelope_rms(y, 4, **bad)
    with pytest.raises(ValueError):
        ctx.envelope_rms(x.double(), 4)
    src, env, rate = ctx.envelope_rms(x, 4), ctx.envelope_rms(x, 8), torch.ones(2, dtype=torch.float64, device=dev)
    ctx.envelope_mix_(x, src, rate, env, 8, 4, 16)                       # (well formed; all rates 1: nothing is touched)
    for args, kw in (((x, src, rate.float(), env, 8, 4, 16), {}), ((x, src, rate, env, 4, 4, 16), {}),      # env too narrow for hop 4
                     ((x, src, rate, env, 8, 4, 64), {}), ((x, src, rate, env, 8, 4, 0), {}),
                     ((x, src, rate, env, 8, 4, 16), dict(owner=_i32(dev, [0]))),
                     ((x, src, rate, env, 8, 4, 16), dict(src_of_row=torch.zeros(2, dtype=torch.int64, device=dev))),
                     ((x, src.float(), rate, env, 8, 4, 16), {}), ((x, src, rate, env, 8, 0, 16), {})):
        with pytest.raises(ValueError):
            ctx.envelope_mix_(*args, **kw)
    torch.cuda.synchronize()
    ctx.poll_error()


# ---- 4. jobs --------------------------------------------------------------------------------------------------------------------
def _hold_signal(got, want, fp32, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    slack = np.abs(want) * 2.0 ** -23 if fp32 else 1e-300
    worst = EC.rel_err(got[want != 0], want[want != 0]) if (want != 0).any() else 0.0
    print(f"{what}: off by at most {worst:.3e} relative (gate {EC.ENV_GATE:g}" + (" + one fp32 ulp)" if fp32 else ")"))
    assert np.isfinite(got).all() and (np.abs(got - want) <= EC.ENV_GATE * np.abs(want) + slack).all()


def test_jobs_with_an_envelope_end_to_end(dev, lib_path, encoder, extractor):
    """Two files (1.3 s in two slices, 0.7 s), three jobs: rate 0.25 (CombSub), rate 0 (Sins), none - a 7-tuple: None in the
    eighth place is refused.  Every span is the same call with 7-tuples followed by the numpy statement on the span and its
    file's audio.  A call whose jobs all have the control switched off (`EnvelopeMix(1.0)`: the three launches run and select
    around every row) is the 7-tuple call, bit for bit.  The hop is 50 ms (2205 samples: a
    workgroup strides a hop-block of the fp64 spans and of the files' fp32 audio).  The leg with an enhancer that changes the
    output's rate is untested: the existing tests have no stub that does."""
    import hipddsp
    import infer_offline
    from infer_offline import EnvelopeMix
    from test_bank_models_host import bank_model
    from test_gpu_many_jobs import _args, _files
    from test_gpu_pitch_tune import _noise
    import synthetic
    SR = synthetic.SR
    models = [bank_model("CombSub", 2, 43, dev), bank_model("Sins", 2, 44, dev)]
    audios, slices = _files()
    env = [EnvelopeMix(0.25, 0.05), EnvelopeMix(0.0, 0.05), None]
    plain = [(0, 0, 1, 0.0, None, None, None), (1, 1, 2, 3.0, None, None, None), (0, 0, 1, 2.0, None, None, None)]
    jobs = [job if e is None else job + (e,) for job, e in zip(plain, env)]
    noise = _noise(dev, slices, jobs)
    run = lambda jj: infer_offline.convert_many_device(None, _args(), audios, SR, encoder, extractor, slices=slices, jobs=jj,  # noqa: E731
                                                       models=models, batch_frames=1, noise=noise)
    ref, ref_spans, _ = run(plain)
    got, spans, sr_o = run(jobs)
    off, off_spans, _ = run([job + (EnvelopeMix(1.0, 0.05),) for job in plain])
    torch.cuda.synchronize()
    hipddsp.context_for(dev).poll_error()
    assert spans == ref_spans == off_spans and sr_o == SR and torch.equal(off, ref)     # all off: the 7-tuple call, bit for bit
    ref, got = ref.cpu().numpy(), got.cpu().numpy()
    span = lambda x, j: x[spans[j][0]:spans[j][0] + spans[j][1]]  # noqa: E731
    hop = env[0].setting(SR)
    assert hop == 2205
    for j in (0, 1):
        want = EC.mix(audios[jobs[j][0]], hop, span(ref, j), hop, 2, env[j].rate)
        _hold_signal(span(got, j), want, False, f"job {j} (rate {env[j].rate})")
        assert np.abs(span(got, j) - span(ref, j)).max() > 1e-4                           # the mix is heard
    assert EC.same_bits(span(got, 2), span(ref, 2)) and np.abs(span(ref, 2)).max() > 1e-3  # the job without one keeps its bits
    outside = np.ones(got.shape, dtype=bool)
    for base, total in spans:
        outside[base:base + total] = False
    assert EC.same_bits(got[outside], ref[outside])
    with pytest.raises(ValueError, match="share hop_seconds and frames"):
        run([jobs[0], plain[1] + (EnvelopeMix(0.5, 0.1),)])


# ---- 5. the bank ----------------------------------------------------------------------------------------------------------------
def _bank_setup():
    from test_gpu_pitch_tune import _bank, _block, _push
    return _bank, _block, _push


def test_bank_envelope_rows(dev, lib_path, encoder):
    """Three slots, slot 1 at rate 0.25 from block 1 on: the graph equals its eager chain to the bit; the slot's gated signal is
    the statement on the bank's window and the signal of the same bank with the slot off; a bank whose slots are all off emits
    the bits of a bank without the feature."""
    import hipddsp
    import synthetic
    _bank, _block, _push = _bank_setup()
    model = synthetic.build_model("CombSub", seed=43, device=dev)[0]
    plain, off = _bank(model, dev, encoder), _bank(model, dev, encoder, envelope=True)
    bank, eager = _bank(model, dev, encoder, envelope=True), _bank(model, dev, encoder, envelope=True, use_graph=False)
    assert plain.graph_builds == bank.graph_builds == 1 and eager.graph_builds == 0
    assert bank.rate_of_slot.dtype == torch.float64 and bank.rate_of_slot.tolist() == [1.0, 1.0, 1.0]
    hop_in, hop_out, m = bank.envelope_setting
    assert (hop_in, hop_out, m) == (int(synthetic.SR * 0.01), int(bank.model_sr * 0.01), 4)
    for k in range(4):
        if k == 1:
            bank.set_envelope(1, 0.25)
            eager.set_envelope(1, 0.25)
        x = _block(k, plain, dev)
        a, o, b, c = _push(plain, x), _push(off, x), _push(bank, x), _push(eager, x)
        torch.cuda.synchronize()
        assert torch.equal(a, o) and torch.equal(plain.last_signal, off.last_signal), k     # all off: the plain bank's bits
        assert torch.equal(b, c) and torch.equal(bank.last_signal, eager.last_signal), k    # the graph against its eager chain
        sig_on, sig_off = bank.bank_graph.sig.cpu().numpy(), off.bank_graph.sig.cpu().numpy()
        if k == 0:
            assert EC.same_bits(sig_on, sig_off)
            continue
        assert EC.same_bits(sig_on[[0, 2]], sig_off[[0, 2]]) and torch.equal(bank.windows, off.windows), k
        want = EC.mix(off.windows[1].cpu().numpy(), hop_in, sig_off[1], hop_out, m, 0.25)
        _hold_signal(sig_on[1], want, True, f"block {k}, slot 1's gated signal")
        assert np.abs(sig_on[1] - sig_off[1]).max() > 1e-5, k
    assert bank.graph_builds == 1 and eager.graph_builds == 0                                 # `set_envelope` captured nothing
    bank.reset(1)
    assert bank.rate_of_slot.tolist() == [1.0, 1.0, 1.0] and bank.graph_builds == 1
    bank.set_envelope(0, 0.5)
    bank.set_envelope(0, None)
    assert bank.rate_of_slot.tolist() == [1.0, 1.0, 1.0]
    for bad in (1.5, -0.1, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="set_envelope"):
            bank.set_envelope(0, bad)
    with pytest.raises(ValueError, match="without envelope=True"):
        plain.set_envelope(0, 0.5)
    hipddsp.context_for(dev).poll_error()


def test_bank_envelope_with_active_widths(dev, lib_path, encoder):
    """`active_widths=(2,)`: a compact row reads its SLOT's rate through the width's row table, a padding row has no owner and
    raises nothing; a paused slot's rate row is unchanged; `set_envelope` captures nothing."""
    import hipddsp
    import synthetic
    _bank, _block, _push = _bank_setup()
    model = synthetic.build_model("CombSub", seed=43, device=dev)[0]
    kw = dict(active_widths=(2,))
    plain, bank, eager = _bank(model, dev, encoder, **kw), _bank(model, dev, encoder, envelope=True, **kw), \
        _bank(model, dev, encoder, envelope=True, use_graph=False, **kw)
    builds = bank.graph_builds
    for b in (bank, eager):
        b.set_envelope(2, 0.25)
        b.set_envelope(1, 0.5)                                                              # slot 1 is paused in every call below
    assert bank.graph_builds == builds
    rates = bank.rate_of_slot.clone()
    for k, active in enumerate(([0, 2], [2], [0, 2], [2])):                                 # ([2] at width 2: a padding row)
        x = _block(k, plain, dev)
        a, b, c = _push(plain, x, active), _push(bank, x, active), _push(eager, x, active)
        torch.cuda.synchronize()
        assert torch.equal(b, c) and b.shape[0] == len(active) and torch.isfinite(b).all(), k
        if len(active) == 2:
            assert torch.equal(a[0], b[0]), k                                               # slot 0 is off: the plain bank's bits
        assert not torch.equal(a[-1], b[-1]), k                                             # slot 2 is mixed
        assert torch.equal(bank.rate_of_slot, rates) and rates.tolist() == [1.0, 0.5, 0.25], k
    assert bank.graph_builds == builds
    hipddsp.context_for(dev).poll_error()
