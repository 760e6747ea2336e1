"""Host side of the active sets of `realtime.StreamBank`: the width ladder (`realtime.active_width`), the refusals of the
constructor and of the push calls, which are raised before anything needs a device, and the two row movers in the header, the
library and the binding."""
import inspect
import os
import re

import pytest
import torch

import synthetic
from conftest import ROOT

NEW = ["ddsp_bank_gather", "ddsp_bank_scatter"]
S = 4


def test_active_width_over_the_ladder():
    import realtime
    ladder = (1, 2, 4)
    assert [realtime.active_width(A, ladder) for A in (1, 2, 3, 4)] == [1, 2, 4, 4]
    assert realtime.active_width(3, (3,)) == 3 and realtime.active_width(5, (2, 8, 16)) == 8
    for bad in (5, 0, -1, True, 2.0):
        with pytest.raises(ValueError):
            realtime.active_width(bad, ladder)
            pytest.fail(f"{bad!r} was accepted")


def _bank(model, **kw):
    """A bank on the CPU: its state is plain tensors, and no call that passes the refusals could run."""
    import realtime
    return realtime.StreamBank(model, S, 44100, 0.2, 0.04, "cpu", buffer_num=4, use_graph=False, **kw)


def test_ladder_of_the_constructor(lib_path):
    model, _ = synthetic.build_model("CombSub", seed=43)
    assert _bank(model).active_widths is None and _bank(model).last_active is None
    assert _bank(model, active_widths=(1, 2)).active_widths == (1, 2, 4)
    assert _bank(model, active_widths=(2, 4)).active_widths == (2, 4)
    assert _bank(model, active_widths=()).active_widths == (4,)
    for bad in ((2, 1), (1, 1), (0, 2), (1, 5), (True, 2), (1.0, 2), 2, "12"):
        with pytest.raises(ValueError):
            _bank(model, active_widths=bad)
            pytest.fail(f"{bad!r} was accepted")


def test_refusals_come_before_any_device_call(lib_path, monkeypatch):
    """A `hipddsp.Context` cannot be made here (no device): every refusal below must be raised before one is asked for, and
    before the row table is written."""
    import hipddsp
    import realtime
    monkeypatch.setattr(hipddsp, "context_for", lambda device: pytest.fail("a refusal reached the device"))
    monkeypatch.setattr(realtime._Rows, "select", lambda self, active: pytest.fail("a refusal reached the row table"))
    model, _ = synthetic.build_model("CombSub", seed=43)
    plain, bank = _bank(model), _bank(model, active_widths=(1, 2))
    Fr, T = bank.frames, bank.frames * 512

    def args(A):
        return torch.zeros(A, bank.block), torch.zeros(A, Fr, 256), torch.full((A, Fr, 1), 220.0)

    with pytest.raises(ValueError):
        plain.push_block(*args(2), active=[1, 3])                       # a bank built without active_widths
    bad_sets = [[], (), [3, 1], [1, 1], [0, 1, 1], [-1, 2], [1, 4], [4], [True], [False, 1], [1.0], [1, 2.0], ["1"],
                [torch.tensor(1)], 3]
    for active in bad_sets:
        A = len(active) if hasattr(active, "__len__") and len(active) else 1
        with pytest.raises(ValueError):
            bank.push_block(*args(A), active=active)
            pytest.fail(f"active={active!r} was accepted")
    blocks, units, f0 = args(2)
    bad_rows = [
        dict(blocks=torch.zeros(S, bank.block)), dict(blocks=torch.zeros(3, bank.block)), dict(blocks=torch.zeros(2, bank.block + 1)),
        dict(blocks=torch.zeros(bank.block)), dict(units=torch.zeros(S, Fr, 256)), dict(units=torch.zeros(2, Fr + 1, 256)),
        dict(f0=torch.zeros(S, Fr, 1)), dict(f0=torch.zeros(2, Fr)), dict(noise=torch.zeros(S, T)), dict(noise=torch.zeros(2, T - 1)),
        dict(rand_ini=torch.zeros(S, 9)), dict(rand_ini=torch.zeros(8)), dict(rand_ini=torch.zeros(3, 9))]
    for kw in bad_rows:
        with pytest.raises(ValueError):
            bank.push_block(**{**dict(blocks=blocks, units=units, f0=f0), **kw}, active=[1, 3])
            pytest.fail(f"{ {k: tuple(v.shape) for k, v in kw.items()} } was accepted")
    with pytest.raises(ValueError):
        bank.push_audio(blocks, active=[1, 3])                          # (a bank without the analysers)
    # the bank is as it was built
    for b in (plain, bank):
        assert not b.windows.any() and not b.sola_buffer.any() and b.last_active is None and b.graph_builds == 0
    assert all(r.rows.tolist() == [-1] * W for W, r in bank._compact.items()) and sorted(bank._compact) == [1, 2, 4]


def test_new_symbols_declared_exported_and_bound(lib_path):
    """(The ABI number stays at 8: the two entry points stand beside unchanged ones.)"""
    import hipddsp
    import realtime
    lib = hipddsp.load_library()
    text = open(os.path.join(ROOT, "include", "ddsp_amd.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in hipddsp.SIGNATURES, name
        assert getattr(lib, name).argtypes == hipddsp.SIGNATURES[name][1]
    with open(os.path.join(ROOT, "ddsp-svc-official_amd", "csrc", "ctx.hip")) as fh:
        src = int(re.search(r"#define DDSP_ABI_VERSION (\d+)", fh.read()).group(1))
    assert hipddsp.ABI_VERSION == 8 == src == lib.ddsp_abi_version()
    for method, name in (("bank_gather_", NEW[0]), ("bank_scatter_", NEW[1])):
        called = re.findall(r"call\(\s*\"(ddsp_\w+)\"", inspect.getsource(getattr(hipddsp.Context, method)))
        assert called == [name], (method, called)
    assert "active_widths" in inspect.signature(realtime.StreamBank.__init__).parameters
    for call in (realtime.StreamBank.push_audio, realtime.StreamBank.push_block):
        assert list(inspect.signature(call).parameters)[-3:] == ["noise", "rand_ini", "active"]
    import graphed
    assert "push" in inspect.signature(graphed.block_chain).parameters
