"""The caller-owned buffer contract of include/avvad.h for avvad_resample and avvad_resample_stream, through the library
itself: outputs and the new stream state sit between guard bands (tests/abi_guard.py) under the three fills; what they hold
on entry reaches no result, nothing outside the documented cells changes, and a refused call leaves every bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_guard as G
import resample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UP, DOWN = 160, 441


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _whole_case(g, taps_off=0, expect=0):
    from avvad import _lib as L, ops
    lens = [1000, 0, 333]
    B, Lmax = 3, 1000
    Lout = R.length(Lmax, UP, DOWN)
    pitch = Lout + 5
    torch.manual_seed(0)
    x = torch.randn(B, Lmax, device=DEV)
    taps = ops.resample_taps_on(UP, DOWN, DEV)
    out = g.workspace(B * pitch, DEV).view(B, pitch)
    n_out = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    rc = L.lib().avvad_resample(_p(x), Lmax, _p(torch.tensor(lens, dtype=torch.int32, device=DEV)),
                                C.c_void_p(taps.data_ptr() + taps_off), UP, DOWN, _p(out), pitch, _p(n_out), B, Lmax, None)
    torch.cuda.synchronize()
    assert rc == expect
    return {"out": out[:, :Lout], "behind": out[:, Lout:], "n_out": n_out}, lens


def test_resample_writes_its_cells_and_nothing_else():
    def case(g):
        res, lens = _whole_case(g)
        behind = res["behind"]                                                        # columns from Lout to the pitch keep the fill
        assert torch.equal(behind.contiguous().view(torch.int32), torch.full_like(behind, g.fill).contiguous().view(torch.int32))
        assert res["n_out"].tolist() == [R.length(n, UP, DOWN) for n in lens]
        return {"out": res["out"], "n_out": res["n_out"]}
    res = G.run_direct(case)
    out = res["out"].cpu().numpy()
    assert np.all(np.isfinite(out)) and np.all(out[1].view(np.int32) == 0)           # an empty row is +0 throughout
    assert np.all(out[2, R.length(333, UP, DOWN):].view(np.int32) == 0)


def _stream_case(g, taps_off=0, expect=0):
    from avvad import _lib as L, ops
    B, n_in = 3, 500
    H = R.params(UP, DOWN)[2]
    torch.manual_seed(1)
    chunk = torch.randn(B, n_in, device=DEV)
    state_in = torch.randn(B, H, device=DEV)
    nv, ib = [500, 0, 123], [700, 40, 0]
    ob = [R.emitted(n, UP, DOWN) for n in ib]
    ne = [R.emitted(ib[0] + nv[0], UP, DOWN) - ob[0], 0, R.length(123, UP, DOWN)]      # goes on, idles, ends
    n_max = max(ne) + 3
    pitch = n_max + 4
    counts = torch.tensor([nv, ib, ob, ne], dtype=torch.int64, device=DEV)
    taps = ops.resample_taps_on(UP, DOWN, DEV)
    out = g.workspace(B * pitch, DEV).view(B, pitch)
    state_out = g.workspace(B * H, DEV).view(B, H)
    rc = L.lib().avvad_resample_stream(_p(chunk), n_in, _p(counts[0]), _p(counts[1]), _p(counts[2]), _p(counts[3]), _p(state_in),
                                       _p(state_out), C.c_void_p(taps.data_ptr() + taps_off), UP, DOWN, _p(out), pitch, B, n_in, n_max,
                                       None)
    torch.cuda.synchronize()
    assert rc == expect
    return {"out": out[:, :n_max], "state": state_out}, out[:, n_max:], (chunk, state_in, nv, ne)


def test_resample_stream_writes_its_cells_and_nothing_else():
    kept = {}

    def case(g):
        res, behind, kept["in"] = _stream_case(g)
        assert torch.equal(behind.contiguous().view(torch.int32), torch.full_like(behind, g.fill).contiguous().view(torch.int32))
        return res
    res = G.run_direct(case)
    chunk, state_in, nv, ne = kept["in"]
    out, state = res["out"], res["state"]
    for b in range(3):
        assert np.all(out[b, ne[b]:].cpu().numpy().view(np.int32) == 0)
        assert bool(torch.isfinite(out[b, :ne[b]]).all())
        want = torch.cat([state_in[b], chunk[b, :nv[b]]])[-state.shape[1]:]            # the last H of state ++ chunk
        assert torch.equal(state[b], want), b


@pytest.mark.parametrize("case", [_whole_case, _stream_case])
def test_misaligned_taps_are_refused_with_every_buffer_intact(case):
    g = G.Guard(float("nan"))
    case(g, taps_off=4, expect=-1)
    g.check()
    g.assert_untouched()
