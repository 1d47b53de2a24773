"""The caller-owned buffer contract of include/avvad.h for the mask-regression losses (avvad_spectral_loss), through
tests/abi_guard.py as tests/test_mix_contract_gpu.py does for its family: zero-, NaN- and 1e30-filled guarded workspaces
and outputs give the same bits with the guards intact; a workspace one float short is refused (AVVAD_EWORKSPACE) with
everything still poisoned; a NULL where a pointer is needed, an unknown kind or pred_mode, a bad shape, bad strides and a
misaligned pointer are refused (AVVAD_EINVAL) before anything is launched; nothing is written outside loss[1],
row_loss[B] and dpred[B * T * F]."""
import ctypes as Ct

import pytest
import torch

import spectral_loss_ref as R
from abi_guard import expect_refused, run_contract, run_direct

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _ops():
    from avvad import ops
    return ops


def _stream():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _inputs(c):
    """pred, target, mix, speech on the GPU, with NaN on every frame at or behind a row's length: none of it may be read"""
    t = {k: c[k].to(DEV).clone() for k in ("pred", "target")}
    t.update({k: torch.view_as_real(c[k].to(DEV)).clone() for k in ("mix", "speech")})
    for b, n in enumerate(R.lens_of(c)):
        for v in t.values():
            v[b, n:] = NAN
    return t


@pytest.mark.parametrize("kind", R.KINDS)
def test_spectral_loss_with_poisoned_buffers(monkeypatch, kind):
    ops = _ops()
    c = R.case("ragged", kind, 2)
    t = _inputs(c)

    def run():
        pred = t["pred"].clone().requires_grad_(True)
        loss, rows = ops.spectral_loss(pred, kind, target=t["target"] if kind != "spectrum" else None,
                                       mix=t["mix"] if kind != "mask" else None, speech=t["speech"] if kind == "spectrum" else None,
                                       lengths=list(c["lengths"]), return_rows=True)
        loss.backward()
        return {"loss": loss.detach().view(1), "rows": rows.view(torch.int64), "dpred": pred.grad}
    got = run_contract(monkeypatch, ops, run)
    R.check_spectral(lambda _: (float(got["loss"]), got["rows"].view(torch.float64).cpu().numpy(), got["dpred"].cpu().numpy()), c)
    # without a gradient to compute: the same loss and rows
    with torch.no_grad():
        only = run_contract(monkeypatch, ops, lambda: {"loss": ops.spectral_loss(
            t["pred"], kind, target=t["target"] if kind != "spectrum" else None, mix=t["mix"] if kind != "mask" else None,
            speech=t["speech"] if kind == "spectrum" else None, lengths=list(c["lengths"])).view(1)})
    assert torch.equal(only["loss"], got["loss"])
    expect_refused(monkeypatch, ops, run, "AVVAD_EINVAL", offset=1)             # the workspace 4 bytes off its alignment


def test_nothing_is_written_outside_the_three_outputs():
    """Through the C ABI with every output inside guards of its own: loss[1], row_loss[B] (2 B floats) and dpred[B T F]"""
    from avvad import _lib as L
    lib = L.lib()
    c = R.case("ragged", "spectrum", 2)
    B, T, F = c["B"], c["T"], c["F"]
    t = _inputs(c)
    lens = torch.tensor(c["lengths"], dtype=torch.int32).to(DEV)
    st = t["mix"].stride()[:3]

    def case(g):
        loss, rows, dpred = g.workspace(1, DEV), g.workspace(2 * B, DEV), g.workspace(B * T * F, DEV)
        ws = g.workspace_bytes(lib.avvad_spectral_loss_workspace(B, T, F), DEV)
        L.check(lib.avvad_spectral_loss(L.ptr(t["pred"]), 2, 2, None, L.ptr(t["mix"]), *st, L.ptr(t["speech"]), *st, L.ptr(lens),
                                        L.ptr(loss), L.ptr(rows), L.ptr(dpred), B, T, F, L.ptr(ws), ws.numel() * 4, _stream()),
                "avvad_spectral_loss")
        return {"loss": loss, "rows": rows.view(torch.int32), "dpred": dpred}
    got = run_direct(case)
    R.check_spectral(lambda _: (float(got["loss"]), got["rows"].view(torch.float64).cpu().numpy(),
                                got["dpred"].view(B, T, F).cpu().numpy()), c)


def test_bad_arguments_are_refused_before_any_launch():
    """Through the C ABI: every refusal leaves the outputs and the workspace as they were; the proper call succeeds."""
    from avvad import _lib as L
    ops = _ops()
    lib = L.lib()
    c = R.case("ragged", "spectrum", 2)
    B, T, F = c["B"], c["T"], c["F"]
    t = _inputs(c)
    lens = torch.tensor(c["lengths"], dtype=torch.int32).to(DEV)
    st = tuple(t["mix"].stride()[:3])
    off4 = lambda v: Ct.c_void_p(v.data_ptr() + 4)          # noqa: E731
    loss = torch.full((1,), NAN, device=DEV)
    rows = torch.full((B + 1,), NAN, dtype=torch.float64, device=DEV)           # room for the shift
    dpred = torch.full((B, T, F), NAN, device=DEV)
    nbytes = lib.avvad_spectral_loss_workspace(B, T, F)
    ws = torch.full((nbytes // 4 + 4,), NAN, device=DEV)

    def call(pred_p=L.ptr(t["pred"]), mode=2, kind=2, target_p=L.ptr(t["target"]), mix_p=L.ptr(t["mix"]), sx=st,
             speech_p=L.ptr(t["speech"]), ss=st, loss_p=L.ptr(loss), rows_p=L.ptr(rows), shape=(B, T, F), ws_p=L.ptr(ws), ws_bytes=nbytes):
        return lib.avvad_spectral_loss(pred_p, mode, kind, target_p, mix_p, *sx, speech_p, *ss, L.ptr(lens), loss_p, rows_p,
                                       L.ptr(dpred), *shape, ws_p, ws_bytes, _stream())
    refused = [(call(ws_bytes=nbytes - 4), -2)]
    refused += [(rc, -1) for rc in (
        call(pred_p=None), call(mix_p=None), call(speech_p=None), call(loss_p=None), call(ws_p=None),
        call(kind=0, target_p=None), call(kind=1, target_p=None), call(kind=1, mix_p=None),
        call(kind=3), call(kind=-1), call(mode=0), call(mode=3),
        call(shape=(0, T, F)), call(shape=(B, 0, F)), call(shape=(B, T, 0)), call(shape=(65536, T, F)), call(shape=(B, 1 << 16, (1 << 14) + 1)),
        call(sx=(st[0], st[1], 3)), call(sx=(st[0], st[1] + 1, 2)), call(sx=(st[0] + 1, st[1], 2)), call(ss=(st[0], st[1], 1)),
        call(sx=(st[0], 0, 2)), call(ss=(st[0], st[1], -2)), call(sx=(0, st[1], 2)),
        call(mix_p=off4(t["mix"])), call(speech_p=off4(t["speech"])), call(rows_p=off4(rows)), call(ws_p=off4(ws)))]
    for rc, want in refused:
        assert rc == want
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for v in (loss, rows, dpred, ws))
    assert call() == 0
    pred = t["pred"].clone().requires_grad_(True)
    want_loss, want_rows = ops.spectral_loss(pred, "spectrum", mix=t["mix"], speech=t["speech"], lengths=list(c["lengths"]),
                                             return_rows=True)
    want_loss.backward()
    assert torch.equal(loss[0], want_loss.detach()) and torch.equal(rows[:B], want_rows) and torch.equal(dpred, pred.grad)
    assert bool(torch.isnan(rows[B])) and bool(torch.isnan(ws[nbytes // 4:]).all())
