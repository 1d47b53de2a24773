"""The caller-owned buffer contract of include/avvad.h for avvad_stoi_loss, through tests/abi_guard.py as
tests/test_stoi_contract_gpu.py does for the score: zero-, NaN- and 1e30-filled guarded workspaces and outputs give the same
bits with the guards intact; a workspace one float short is refused (AVVAD_EWORKSPACE) with everything still poisoned; a
workspace, a score array or a tap table 4 bytes off its alignment and a row pitch below L are refused (AVVAD_EINVAL) before
anything is launched."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import stoi_loss_ref as G
import stoi_ref as R
from abi_guard import expect_refused, run_contract

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
T_ = torch.tensor


def _ops():
    from avvad import ops
    return ops


def _stream():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ragged(names):
    """rows of one rate at a pitch 77 floats wider than the longest, NaN behind the lengths, and an empty row at the end"""
    L = max(R.case(n)[1].size for n in names)
    x = np.full((len(names) + 1, L + 77), NAN, dtype=np.float32)
    y = x.copy()
    lengths = []
    for b, n in enumerate(names):
        _, cx, cy = R.case(n)
        x[b, :cx.size], y[b, :cx.size] = cx, cy
        lengths.append(cx.size)
    return T_(x).to(DEV)[:, :L], T_(y).to(DEV)[:, :L], lengths + [0]


@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("fs, names", [(10000, ["k10_9001_half", "k10_4097_one_segment", "k10_4096_no_segment"]),
                                       (16000, ["k16_11999", "k16_9731"])])
def test_stoi_loss_with_poisoned_buffers(monkeypatch, fs, names, which):
    ops = _ops()
    x, y, lengths = _ragged(names)

    def case():
        yd = y.clone().requires_grad_(True)
        loss, d = ops.stoi_loss(yd, x, lengths=lengths, fs=fs, extended=which == 2, return_scores=True)
        loss.backward()
        return {"loss": loss.detach().view(1), "d": d.view(torch.int64), "grad": yd.grad}
    got = run_contract(monkeypatch, ops, case)
    d, grad = got["d"].view(torch.float64).cpu().numpy(), got["grad"].cpu().numpy()
    key = "stoi" if which == 1 else "estoi"
    for b, n in enumerate(names):
        ref = R.reference(n)
        assert abs(d[b] - ref[key]) <= R.GPU_BOUND
        assert not grad[b, lengths[b]:].any()
        if ref["segments"] == 0:
            assert d[b] == 1e-5 and not grad[b].any()
        elif n in G.grad_cases(which):
            assert G.err(grad[b, :lengths[b]], G.reference(n, which)[1]) <= G.GPU_GRAD_BOUND
    assert d[-1] == 1e-5 and not grad[-1].any()
    # the workspace 4 bytes off its alignment
    expect_refused(monkeypatch, ops, case, "AVVAD_EINVAL", offset=1)


def test_misaligned_pointers_and_short_pitches_are_refused():
    """Through the C ABI: d / taps 4 bytes off their 8-byte alignment, the workspace 4 bytes off and a pitch below L return
    AVVAD_EINVAL, a workspace 4 bytes short AVVAD_EWORKSPACE, and nothing has changed; the proper call succeeds."""
    from avvad import _lib as L
    ops = _ops()
    lib = L.lib()
    off4 = lambda t: Ct.c_void_p(t.data_ptr() + 4)          # noqa: E731
    fs, x, y = R.case("k16_9218")
    n = x.size
    xd, yd = T_(x).to(DEV), T_(y).to(DEV)
    taps = torch.zeros(162, dtype=torch.float64, device=DEV)
    taps[:161] = T_(ops.stoi_taps()).to(DEV)
    d = torch.full((2,), NAN, dtype=torch.float64, device=DEV)                # room for the shifted pointer
    info = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    loss = torch.full((1,), NAN, device=DEV)
    dproc = torch.full((n + 3,), NAN, device=DEV)
    nbytes = lib.avvad_stoi_loss_workspace(1, n, fs)
    ws = torch.full((nbytes // 4 + 4,), NAN, device=DEV)

    def call(d_p=None, taps_p=None, ws_p=None, ws_bytes=nbytes, ld_x=n, ld_y=n, ld_g=n):
        return lib.avvad_stoi_loss(L.ptr(xd), ld_x, L.ptr(yd), ld_y, None, taps_p or L.ptr(taps), 1, n, fs, 2, L.ptr(loss),
                                   d_p or L.ptr(d), L.ptr(info), L.ptr(dproc), ld_g, ws_p or L.ptr(ws), ws_bytes, _stream())
    for rc, want in ((call(d_p=off4(d)), -1), (call(taps_p=off4(taps)), -1), (call(ws_p=off4(ws)), -1), (call(ld_x=n - 1), -1),
                     (call(ld_y=n - 1), -1), (call(ld_g=n - 1), -1), (call(ws_bytes=nbytes - 4), -2)):
        assert rc == want
        assert bool(torch.isnan(d).all()) and bool(torch.isnan(ws).all()) and info.tolist() == [-7] * 3
        assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dproc).all())
    assert call() == 0
    ref = R.reference("k16_9218")
    assert info.tolist() == [ref["frames"], ref["kept"], ref["segments"]]
    assert abs(float(d[0]) - ref["estoi"]) <= R.GPU_BOUND and bool(torch.isnan(d[1]))
    assert float(loss) == float(np.float32(-float(d[0])))
    assert G.err(dproc[:n].cpu().numpy(), G.reference("k16_9218", 2)[1]) <= G.GPU_GRAD_BOUND and bool(torch.isnan(dproc[n:]).all())
    assert bool(torch.isnan(ws[nbytes // 4:]).all())
