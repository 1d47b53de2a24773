"""The caller-owned buffer contract of include/avvad.h for the SI-SDR training entry points (avvad_istft_bwd,
avvad_resynth_bwd, avvad_si_sdr_loss), through tests/abi_guard.py as tests/test_score_contract_gpu.py does for its family:
zero-, NaN- and 1e30-filled guarded workspaces and outputs give the same bits with the guards intact; a workspace one float
short is refused (AVVAD_EWORKSPACE) with everything still poisoned; a workspace 4 bytes off its alignment, mask modes 0 and
3 on the backward calls and a ``ratios`` 4 bytes off its 8-byte alignment are refused (AVVAD_EINVAL) before anything is
launched.  The cases call the library themselves, with buffers from the guarded ``ops._ws`` / ``ops.torch.empty``; the path
through autograd gets its short run from ``expect_backward_refused``."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import sisdr_ref as S
from abi_guard import expect_backward_refused, expect_refused, run_contract

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_ = torch.from_numpy
N_FFT, HOP, FRAMES = 64, 16, (9, 4, 1)


def _ops():
    from avvad import ops
    return ops


def _stream():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _inputs():
    """the ragged 64 / 16 case of tests/test_sisdr_gpu.py, NaN in every padding"""
    case = S.cached_istft_case(N_FFT, HOP, FRAMES, 2, True, 100 + N_FFT + HOP)
    dev = {k: T_(case[k]).to(DEV) for k in ("spec", "mask", "dout")}
    dev["frames"] = torch.tensor(case["frames"], dtype=torch.int32, device=DEV)
    dev["lengths"] = torch.tensor(case["lengths"], dtype=torch.int32, device=DEV)
    return case, dev


def _istft_bwd(dev, mode=2, ws_mode=None):
    """avvad_istft_bwd through the C ABI (``ws_mode``: the mode the workspace is sized for, where ``mode`` has no size)"""
    ops = _ops()
    L, lib = ops.L, ops.L.lib()
    B, T, F = dev["mask"].shape
    mk = lambda m: L.IstftDesc(B, T, N_FFT, HOP, N_FFT // 2, dev["dout"].shape[1], m)          # noqa: E731
    d = mk(mode)
    ws = ops._ws(lib.avvad_istft_bwd_workspace(Ct.byref(mk(mode if ws_mode is None else ws_mode))), DEV)
    dmask = ops.torch.empty(B, T, F, dtype=torch.float32, device=DEV)
    L.check(lib.avvad_istft_bwd(L.ptr(dev["spec"]), T * F * 2, F * 2, 2, L.ptr(dev["mask"]), L.ptr(dev["frames"]), L.ptr(dev["lengths"]),
                                None, L.ptr(dev["dout"]), L.ptr(dmask), Ct.byref(d), L.ptr(ws), ws.numel() * 4, _stream()),
            "avvad_istft_bwd")
    return {"dmask": dmask}


def test_istft_bwd_with_poisoned_buffers(monkeypatch):
    ops = _ops()
    case, dev = _inputs()
    got = run_contract(monkeypatch, ops, lambda: _istft_bwd(dev))
    S.check_dmask(lambda c: got["dmask"].cpu().numpy(), case, name="contract: avvad_istft_bwd")
    expect_refused(monkeypatch, ops, lambda: _istft_bwd(dev), "AVVAD_EINVAL", offset=1)
    for mode in (0, 3):
        expect_refused(monkeypatch, ops, lambda: _istft_bwd(dev, mode=mode, ws_mode=2), "AVVAD_EINVAL")
        d = ops.L.IstftDesc(3, 9, N_FFT, HOP, 0, 100, mode)
        assert ops.L.lib().avvad_istft_bwd_workspace(Ct.byref(d)) == 0


def _wave_inputs():
    ops = _ops()
    lens = [700, 431]
    rng = np.random.default_rng(41)
    wave = np.zeros((2, 700), dtype=np.float32)
    for b, n in enumerate(lens):
        wave[b, :n] = rng.standard_normal(n) * 0.3
    frames = [ops.n_frames(n, N_FFT, HOP) for n in lens]
    T, F = max(frames), N_FFT // 2 + 1
    logits = rng.standard_normal((2, T, F)).astype(np.float32)
    dout = rng.standard_normal((2, 700)).astype(np.float32)
    dout[:, :N_FFT - HOP] = 0
    for b, n in enumerate(lens):
        dout[b, n - (N_FFT - HOP):n] = 0
        dout[b, n:] = np.nan
        logits[b, frames[b]:] = np.nan
    return lens, frames, T_(wave).to(DEV), T_(logits).to(DEV), T_(dout).to(DEV)


def _resynth_bwd(wave, logits, frames, lens, dout, mode=2, ws_mode=None):
    ops = _ops()
    L, lib = ops.L, ops.L.lib()
    B, T, F = logits.shape
    sd = L.StftDesc(B, wave.shape[1], N_FFT, HOP, T, 0.0)
    mk = lambda m: L.IstftDesc(B, T, N_FFT, HOP, 0, wave.shape[1], m)          # noqa: E731
    d = mk(mode)
    ws = ops._ws(lib.avvad_resynth_bwd_workspace(Ct.byref(sd), Ct.byref(mk(mode if ws_mode is None else ws_mode))), DEV)
    dmask = ops.torch.empty(B, T, F, dtype=torch.float32, device=DEV)
    nf = torch.tensor(frames, dtype=torch.int32, device=DEV)
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
    L.check(lib.avvad_resynth_bwd(L.ptr(wave), L.ptr(logits), L.ptr(nf), L.ptr(ln), None, L.ptr(dout), L.ptr(dmask), Ct.byref(sd),
                                  Ct.byref(d), L.ptr(ws), ws.numel() * 4, _stream()), "avvad_resynth_bwd")
    return {"dmask": dmask}


def test_resynth_bwd_with_poisoned_buffers(monkeypatch):
    ops = _ops()
    lens, frames, wave, logits, dout = _wave_inputs()
    case = lambda **k: _resynth_bwd(wave, logits, frames, lens, dout, **k)          # noqa: E731
    got = run_contract(monkeypatch, ops, case)
    # the same gradient through autograd, from logits whose padding is finite
    m = torch.nan_to_num(logits).requires_grad_(True)
    ops.resynth(wave, m, mask_mode=2, n_fft=N_FFT, hop=HOP, sample_lengths=lens).backward(dout)
    assert torch.equal(m.grad, got["dmask"])
    for b, nf in enumerate(frames):
        assert torch.count_nonzero(got["dmask"][b, nf:]).item() == 0 and torch.count_nonzero(got["dmask"][b, :nf]).item() > 0
    expect_refused(monkeypatch, ops, case, "AVVAD_EINVAL", offset=1)
    for mode in (0, 3):
        expect_refused(monkeypatch, ops, lambda: case(mode=mode, ws_mode=2), "AVVAD_EINVAL")


def test_backward_through_autograd_is_refused_with_a_short_workspace(monkeypatch):
    ops = _ops()
    lens, frames, wave, logits, dout = _wave_inputs()
    spec = ops.stft_complex(wave, N_FFT, HOP)

    def resynth():
        m = torch.nan_to_num(logits).requires_grad_(True)
        return ops.resynth(wave, m, mask_mode=2, n_fft=N_FFT, hop=HOP, sample_lengths=lens)

    def istft():
        m = torch.nan_to_num(logits).requires_grad_(True)
        return ops.istft(spec, N_FFT, HOP, mask=m, mask_mode=2, n_frames=frames, length=lens)
    for entry, forward in (("avvad_resynth_bwd", resynth), ("avvad_istft_bwd", istft)):
        expect_backward_refused(monkeypatch, ops, entry, forward, lambda out: out.backward(dout))
        expect_backward_refused(monkeypatch, ops, entry, forward, lambda out: out.backward(dout), match="AVVAD_EINVAL", misaligned=True)


def _loss(case, ratios_off=0):
    """avvad_si_sdr_loss through the C ABI on NaN-padded rows; ``ratios_off``: bytes by which ratios is moved"""
    ops = _ops()
    L, lib = ops.L, ops.L.lib()
    est, ref = case["dev"]
    B, P = est.shape
    ws = ops._ws(lib.avvad_si_sdr_loss_workspace(B, P), DEV)
    loss = ops.torch.empty(1, dtype=torch.float32, device=DEV)
    dest = ops.torch.empty(B, P, dtype=torch.float32, device=DEV)
    ratios = ops.torch.empty(2 * B + 2, dtype=torch.float32, device=DEV)            # B doubles and room for the shifted pointer
    L.check(lib.avvad_si_sdr_loss(L.ptr(est), P, L.ptr(ref), P, L.ptr(case["lens32"]), L.ptr(loss), Ct.c_void_p(ratios.data_ptr() + ratios_off),
                                  L.ptr(dest), P, B, P, L.ptr(ws), ws.numel() * 4, _stream()), "avvad_si_sdr_loss")
    return {"loss": loss, "dest": dest, "ratios": ratios[:2 * B].view(torch.int32)}            # (an empty row's ratio is NaN: bits)


def test_si_sdr_loss_with_poisoned_buffers(monkeypatch):
    ops = _ops()
    P = ops.SCORE_CHUNK + 77
    case = S.sisdr_case([P, 300, 0], P, 0, 0, seed=43)
    case["dev"] = (T_(case["est"]).to(DEV), T_(case["ref"]).to(DEV))
    case["lens32"] = torch.tensor(case["lengths"], dtype=torch.int32, device=DEV)
    got = run_contract(monkeypatch, ops, lambda: _loss(case))
    ratios = got["ratios"].view(torch.float32).contiguous().view(torch.float64).cpu().numpy()
    S.check_sisdr(lambda c: (float(got["loss"]), ratios, got["dest"].cpu().numpy()), case, name="contract: avvad_si_sdr_loss")
    assert np.isnan(ratios[2])
    expect_refused(monkeypatch, ops, lambda: _loss(case), "AVVAD_EINVAL", offset=1)
    expect_refused(monkeypatch, ops, lambda: _loss(case, ratios_off=4), "AVVAD_EINVAL")
    # and through ops, the gradient included
    est = case["dev"][0]

    def through_ops():
        e = est.clone().requires_grad_(True)
        loss, r = ops.si_sdr_loss(e, case["dev"][1], case["lengths"], 24, 36, return_ratios=True)
        loss.backward()
        return {"loss": loss.detach(), "ratios": r.view(torch.int64), "grad": e.grad}
    run_contract(monkeypatch, ops, through_ops)
