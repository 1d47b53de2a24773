"""The caller-owned buffer contract of include/avvad.h for the SNR mix (avvad_mix), through tests/abi_guard.py as
tests/test_score_contract_gpu.py does for its family: zero-, NaN- and 1e30-filled guarded workspaces and outputs give
the same bits with the guards intact; a workspace one float short is refused (AVVAD_EWORKSPACE) with everything still
poisoned; a workspace 4 bytes off its alignment, a ratio or an energies array 4 bytes off its 8 bytes, a pitch below L
and an output that is the input are refused (AVVAD_EINVAL) before anything is launched."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import mix_ref
from abi_guard import expect_refused, run_contract

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
ROWS = (0, 4, 7, 8, 10, 11)          # empty, one wrap, many wraps, four chunks, silent noise, silent speech


def _ops():
    from avvad import ops
    return ops


def _stream():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _inputs():
    ops = _ops()
    case = mix_ref.rows_of(mix_ref.ragged_case(), ROWS)
    host = case["clean"].copy()
    for b, n in enumerate(case["lengths"]):
        host[b, n:] = NAN
    return case, torch.from_numpy(host).to(DEV), ops.NoiseBank([torch.from_numpy(c) for c in mix_ref.clips()], DEV)


def test_mix_with_poisoned_buffers(monkeypatch):
    ops = _ops()
    case, clean, bank = _inputs()

    def run():
        noisy, noise, info = ops.mix(clean, case["lengths"], bank, case["clip"], case["start"], case["snr_db"], return_noise=True,
                                     return_info=True)
        return {"noisy": noisy, "noise": noise, "gain": info["gain"], "peak": info["peak"],
                "energies": info["energies"].view(torch.int64)}
    got = run_contract(monkeypatch, ops, run)
    got["energies"] = got["energies"].view(torch.float64)
    mix_ref.check(lambda c: {k: v.cpu().numpy() for k, v in got.items()}, case)
    # without the optional outputs: the same mixture
    only = run_contract(monkeypatch, ops, lambda: {"noisy": ops.mix(clean, case["lengths"], bank, case["clip"], case["start"],
                                                                     case["snr_db"])})
    assert torch.equal(only["noisy"], got["noisy"])
    # the workspace 4 bytes off its alignment
    expect_refused(monkeypatch, ops, run, "AVVAD_EINVAL", offset=1)


def test_misaligned_arrays_short_pitches_and_aliases_are_refused():
    """Through the C ABI: every refusal leaves the outputs and the workspace as they were; the proper call succeeds."""
    from avvad import _lib as L
    ops = _ops()
    lib = L.lib()
    case, clean, bank = _inputs()
    B, n = clean.shape
    off4 = lambda t: Ct.c_void_p(t.data_ptr() + 4)          # noqa: E731
    idx = torch.tensor([case["lengths"], case["clip"], case["start"]], dtype=torch.int32).to(DEV)
    ratio = torch.tensor([ops.mix_ratio(v) for v in case["snr_db"]] + [1.0], dtype=torch.float64).to(DEV)   # room for the shift
    noisy = torch.full((B, n), NAN, device=DEV)
    noise = torch.full((B, n), NAN, device=DEV)
    energies = torch.full((B + 1, 2), NAN, dtype=torch.float64, device=DEV)
    ws = torch.full((lib.avvad_mix_workspace(B, n) // 4,), NAN, device=DEV)

    def call(clean_p=L.ptr(clean), ld=n, ratio_p=L.ptr(ratio), noisy_p=L.ptr(noisy), ld_y=n, noise_p=L.ptr(noise), ld_z=n,
             energies_p=L.ptr(energies), K=bank.K, ws_bytes=ws.numel() * 4):
        return lib.avvad_mix(clean_p, ld, L.ptr(idx[0]), L.ptr(bank.data), bank.data.numel(), L.ptr(bank.clip_off),
                             L.ptr(bank.clip_len), K, L.ptr(idx[1]), L.ptr(idx[2]), ratio_p, noisy_p, ld_y, noise_p, ld_z, None,
                             energies_p, None, B, n, L.ptr(ws), ws_bytes, _stream())
    for rc, want in ((call(ratio_p=off4(ratio)), -1), (call(energies_p=off4(energies)), -1), (call(ld=n - 1), -1),
                     (call(ld_y=n - 1), -1), (call(ld_z=n - 1), -1), (call(K=0), -1), (call(noisy_p=L.ptr(clean)), -1),
                     (call(noise_p=L.ptr(noisy)), -1), (call(ws_bytes=ws.numel() * 4 - 4), -2)):
        assert rc == want
        assert bool(torch.isnan(noisy).all()) and bool(torch.isnan(noise).all()) and bool(torch.isnan(ws).all())
        assert bool(torch.isnan(energies).all())
    assert call() == 0
    want = ops.mix(clean, case["lengths"], bank, case["clip"], case["start"], case["snr_db"], return_noise=True, return_info=True)
    assert torch.equal(noisy, want[0]) and torch.equal(noise, want[1]) and torch.equal(energies[:B], want[2]["energies"])
    assert bool(torch.isnan(energies[B]).all())
    # NULL lengths: every row is L samples long (the NaN behind the lengths is then speech, and stays in its row)
    assert lib.avvad_mix(L.ptr(clean), n, None, L.ptr(bank.data), bank.data.numel(), L.ptr(bank.clip_off), L.ptr(bank.clip_len),
                         bank.K, L.ptr(idx[1]), L.ptr(idx[2]), L.ptr(ratio), L.ptr(noisy), n, None, 0, None, None, None, B, n,
                         L.ptr(ws), ws.numel() * 4, _stream()) == 0
    full = [b for b, m in enumerate(case["lengths"]) if m == n]
    assert not full and bool(torch.isnan(noisy).any(dim=1).all())
