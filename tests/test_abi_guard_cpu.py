"""The buffer-contract harness (tests/abi_guard.py) must be able to FAIL: fake "ops" in plain torch on CPU tensors, one
per way of breaking the contract of include/avvad.h, and a well-behaved one that passes."""
import types

import pytest
import torch

import abi_guard
from abi_guard import GUARD, Guard, GuardError, expect_backward_refused, run_contract


class FakeError(RuntimeError):
    pass


def make_ops(flaw=None):
    """A stand-in for ``avvad.ops`` with one operation, ``double_plus_one(x)``: it stages 2x in a workspace of x.numel()
    floats and writes 2x/2 + 1 to a fresh output.  ``flaw`` selects how it misbehaves."""
    m = types.ModuleType("fake_ops")
    m.torch = torch
    m.L = types.SimpleNamespace(AvvadError=FakeError)
    m._ws = lambda nbytes, device: m.torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
    m.engine_ws = lambda device: m.torch.empty(64, dtype=torch.float32, device=device)

    def raw(ws, index):                      # one float of the workspace's underlying storage, in or out of bounds
        return ws.as_strided((1,), (1,), ws.storage_offset() + index)

    def double_plus_one(x):
        n = x.numel()
        ws = m._ws(4 * n, x.device)
        out = m.torch.empty_like(x)
        if flaw == "launch_then_refuse":
            out[0] = 1.0
        if ws.numel() < n and flaw != "never_refuses":
            raise FakeError("fake op failed: AVVAD_EWORKSPACE (workspace too small)")
        k = min(n, ws.numel())
        if flaw == "reads_workspace":
            out.copy_(x + 1 + 0 * ws[:1])    # 0 * stale: 0 for zeros and 1e30, NaN for NaN
            return out
        if flaw == "reads_workspace_finite":
            out.copy_(x + 1 + (ws[:1] != 0).float())   # a flag word: zero vs "anything else"
            return out
        ws[:k] = 2 * x.reshape(-1)[:k]
        if flaw == "before":
            raw(ws, -1).fill_(3.0)
        if flaw == "behind":
            raw(ws, ws.numel()).fill_(3.0)
        if flaw == "far_behind":
            raw(ws, ws.numel() + GUARD - 1).fill_(3.0)
        if k < n:                            # (never_refuses: goes on with what it was given)
            out.copy_(x + 1)
            return out
        res = ws[:k].view_as(x) / 2 + 1
        if flaw == "unwritten":
            out.reshape(-1)[:-1] = res.reshape(-1)[:-1]
        else:
            out.copy_(res)
        return out
    m.double_plus_one = double_plus_one
    return m


X = torch.arange(12, dtype=torch.float32).reshape(3, 4)


def _run(monkeypatch, flaw):
    ops = make_ops(flaw)
    return run_contract(monkeypatch, ops, lambda: {"y": ops.double_plus_one(X)}, error=FakeError, engine_floats=64)


def test_well_behaved_fake_passes(monkeypatch):
    ops = make_ops()
    res = _run(monkeypatch, None)
    assert torch.equal(res["y"], X + 1)
    assert ops.torch is torch                  # (the patch is gone afterwards, and was never on the real module)


@pytest.mark.parametrize("flaw,what", [("before", "written BEFORE"), ("behind", "written BEHIND"), ("far_behind", "written BEHIND")])
def test_write_outside_the_workspace_is_caught(monkeypatch, flaw, what):
    with pytest.raises(GuardError, match=what):
        _run(monkeypatch, flaw)


def test_unwritten_output_element_is_caught(monkeypatch):
    with pytest.raises(GuardError, match=r"fill 'nan' changes a result.*y: 1 of 12 values differ"):
        _run(monkeypatch, "unwritten")


@pytest.mark.parametrize("flaw,fill", [("reads_workspace", "nan"), ("reads_workspace_finite", "nan")])
def test_result_that_depends_on_the_fill_is_caught(monkeypatch, flaw, fill):
    with pytest.raises(GuardError, match="fill %r changes a result" % fill):
        _run(monkeypatch, flaw)


def test_finite_poison_catches_what_nan_hides(monkeypatch):
    """max(stale, x) swallows a NaN (fmaxf(NaN, x) = x): only the 1e30 run shows it."""
    ops = make_ops()

    def relu_like(x):
        ws = ops._ws(4 * x.numel(), x.device)
        if ws.numel() < x.numel():
            raise FakeError("AVVAD_EWORKSPACE")
        out = ops.torch.empty_like(x)
        out.copy_(torch.fmax(ws.view_as(x), x))
        return out
    with pytest.raises(GuardError, match="fill 'big' changes a result"):
        run_contract(monkeypatch, ops, lambda: {"y": relu_like(X + 1)}, error=FakeError, engine_floats=64)


def test_launch_after_a_short_workspace_is_caught(monkeypatch):
    with pytest.raises(GuardError, match="changed although the call was refused"):
        _run(monkeypatch, "launch_then_refuse")


def test_short_workspace_that_is_not_refused_is_caught(monkeypatch):
    with pytest.raises(GuardError, match="NOT refused"):
        _run(monkeypatch, "never_refuses")


def test_every_entry_point_of_a_case_gets_its_own_short_run(monkeypatch):
    """A refused call raises, so in a case of two operations the second never sees the short workspace: named in
    ``short_ops`` it does, and a launch before its refusal is caught."""
    good, bad = make_ops(), make_ops("launch_then_refuse")
    bad._ws, bad.engine_ws = (lambda *a: good._ws(*a)), (lambda *a: good.engine_ws(*a))   # (one module is patched: good's)
    bad.torch = types.SimpleNamespace(empty_like=lambda *a, **k: good.torch.empty_like(*a, **k))
    case = lambda: {"y": good.double_plus_one(X), "z": bad.double_plus_one(X)}
    kw = dict(error=FakeError, engine_floats=64)
    run_contract(monkeypatch, good, case, **kw)                # the flaw hides behind the first operation's refusal
    with pytest.raises(GuardError, match="second: .*changed although the call was refused"):
        run_contract(monkeypatch, good, case, short_ops={"first": lambda: good.double_plus_one(X),
                                                         "second": lambda: bad.double_plus_one(X)}, **kw)


def _fake_backward(flaw=None):
    """``make_ops()`` with a backward that hands the forward's workspace to a fake library entry point ``fake_bwd(ws, dx,
    ws_bytes, stream)``, as ``avvad.ops`` does with ``ctx``."""
    ops = make_ops()

    def fake_bwd(ws, dx, ws_bytes, stream):
        if flaw == "launch_then_refuse":
            dx[0] = 1.0
        if flaw == "scribbles_on_workspace":
            ws[0] = 5.0
        if ws_bytes < 4 * ws.numel() and flaw != "never_refuses":
            return -2
        dx.copy_(ws / 2)
        return 0
    handle = types.SimpleNamespace(fake_bwd=fake_bwd)
    ops.L.lib = lambda: handle

    def forward():
        ws = ops._ws(4 * X.numel(), X.device)
        ws.copy_(2 * X.reshape(-1))
        return ws

    def backward(ws):
        dx = ops.torch.empty(X.numel())
        if ops.L.lib().fake_bwd(ws, dx, ws.numel() * 4, None):
            raise FakeError("fake_bwd failed: AVVAD_EWORKSPACE (workspace too small)")
        return dx
    return ops, forward, backward


def test_backward_short_run_passes_a_well_behaved_fake_and_leaves_the_library_alone(monkeypatch):
    ops, forward, backward = _fake_backward()
    real = ops.L.lib().fake_bwd
    expect_backward_refused(monkeypatch, ops, "fake_bwd", forward, backward)
    assert ops.L.lib().fake_bwd is real
    assert torch.equal(backward(forward()), X.reshape(-1))


@pytest.mark.parametrize("flaw,what", [("launch_then_refuse", "launched before it refused"), ("scribbles_on_workspace", "launched before it refused"),
                                       ("never_refuses", "NOT refused")])
def test_backward_short_run_catches(monkeypatch, flaw, what):
    ops, forward, backward = _fake_backward(flaw)
    with pytest.raises(GuardError, match=what):
        expect_backward_refused(monkeypatch, ops, "fake_bwd", forward, backward)


def test_backward_short_run_that_never_reaches_the_entry_point_is_caught(monkeypatch):
    ops, forward, _ = _fake_backward()

    def backward(ws):
        raise FakeError("AVVAD_EWORKSPACE, but from somewhere else")
    with pytest.raises(GuardError, match="never reached"):
        expect_backward_refused(monkeypatch, ops, "fake_bwd", forward, backward)


def test_guard_geometry_and_direct_use():
    """The direct-ABI form: alignment of the view, the short mode's size, bit-exact guard check (-0.0 is not 0.0)."""
    g = Guard(0.0)
    ws = g.workspace(100, "cpu")
    assert ws.numel() == 100 and ws.storage_offset() == GUARD and GUARD % 64 == 0
    out = g.new_output(2, 3, device="cpu")
    assert float(out.abs().sum()) == 0
    g.check()
    g.assert_untouched()
    owner = g.workspaces[0][0]
    owner[GUARD - 1] = -0.0                    # equal as a float, not as bits
    with pytest.raises(GuardError, match="BEFORE"):
        g.check()
    gs = Guard(float("nan"), short=True)
    assert gs.workspace_bytes(402, "cpu").numel() == 100       # ceil(402 / 4) - 1: fewer bytes than asked for
    gs.check()
    gs.workspaces[0][0][GUARD + 100] = float("nan")            # same NaN bits: still intact
    gs.check()
    gs.workspaces[0][0][GUARD + 100] = 1.0
    with pytest.raises(GuardError, match="BEHIND"):
        gs.check()
    assert abi_guard.FILLS[2][1] == 1e30
