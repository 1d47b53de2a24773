"""The caller-owned buffer contract of include/avvad.h for avvad_stoi, through tests/abi_guard.py as
tests/test_score_contract_gpu.py does for its family: zero-, NaN- and 1e30-filled guarded workspaces give the same bits with
the guards intact; a workspace one float short is refused (AVVAD_EWORKSPACE) with everything still poisoned; a workspace,
a score array or a tap table 4 bytes off its alignment and a row pitch below L are refused (AVVAD_EINVAL) before anything
is launched."""
import ctypes as Ct

import numpy as np
import pytest
import torch

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


@pytest.mark.parametrize("fs, names", [(10000, ["k10_9001_half", "k10_4097_one_segment", "k10_4096_no_segment"]),
                                       (16000, ["k16_11999", "k16_9731"])])
def test_stoi_with_poisoned_buffers(monkeypatch, fs, names):
    ops = _ops()
    x, y, lengths = _ragged(names)

    def case():
        d, info = ops.stoi(x, y, lengths=lengths, fs=fs, both=True, return_info=True)
        return {"d": d.view(torch.int64), "info": info}
    got = run_contract(monkeypatch, ops, case)
    d, info = got["d"].view(torch.float64).cpu().numpy(), got["info"].cpu().numpy()
    for b, n in enumerate(names):
        ref = R.reference(n)
        assert info[b].tolist() == [ref["frames"], ref["kept"], ref["segments"]]
        assert max(abs(d[b, 0] - ref["stoi"]), abs(d[b, 1] - ref["estoi"])) <= R.GPU_BOUND
    assert info[-1].tolist() == [0, 0, 0] and d[-1].tolist() == [1e-5, 1e-5]
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
    d = torch.full((3,), NAN, dtype=torch.float64, device=DEV)                # room for the shifted pointer
    info = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    nbytes = lib.avvad_stoi_workspace(1, n, fs)
    ws = torch.full((nbytes // 4 + 4,), NAN, device=DEV)

    def call(d_p=None, taps_p=None, ws_p=None, ws_bytes=nbytes, ld_x=n, ld_y=n):
        return lib.avvad_stoi(L.ptr(xd), ld_x, L.ptr(yd), ld_y, None, taps_p or L.ptr(taps), 1, n, fs, 3, d_p or L.ptr(d),
                              L.ptr(info), ws_p or L.ptr(ws), ws_bytes, _stream())
    for rc, want in ((call(d_p=off4(d)), -1), (call(taps_p=off4(taps)), -1), (call(ws_p=off4(ws)), -1), (call(ld_x=n - 1), -1),
                     (call(ld_y=n - 1), -1), (call(ws_bytes=nbytes - 4), -2)):
        assert rc == want
        assert bool(torch.isnan(d).all()) and bool(torch.isnan(ws).all()) and info.tolist() == [-7] * 3
    assert call() == 0
    ref = R.reference("k16_9218")
    assert info.tolist() == [ref["frames"], ref["kept"], ref["segments"]]
    assert max(abs(float(d[0]) - ref["stoi"]), abs(float(d[1]) - ref["estoi"])) <= R.GPU_BOUND and bool(torch.isnan(d[2]))
    assert bool(torch.isnan(ws[nbytes // 4:]).all())
