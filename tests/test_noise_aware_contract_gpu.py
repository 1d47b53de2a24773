"""The caller-owned buffer contract of include/avvad.h for the noise-aware masks (avvad_target_noise_aware and
avvad_target_noise_aware_from_spectrum), through tests/abi_guard.py as tests/test_mix_contract_gpu.py does for its
family: zero-, NaN- and 1e30-filled guarded workspaces and outputs give the same bits with the guards intact; a workspace
one float short is refused (AVVAD_EWORKSPACE) with everything still poisoned; a workspace or a table 4 bytes off its
alignment, odd strides, cuts outside the bins and a call without any output are refused (AVVAD_EINVAL) before anything
is launched."""
import ctypes as Ct

import pytest
import torch

from abi_guard import expect_refused, run_contract
from test_noise_aware_gpu import F, NAMES, _check_exact, _np_complex, _ragged, _spectra

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _ops():
    from avvad import ops
    return ops


def _stream():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_both_entry_points_with_poisoned_buffers(monkeypatch):
    ops = _ops()
    lens, speech, noise = _ragged()
    s, n = torch.from_numpy(speech).to(DEV), torch.from_numpy(noise).to(DEV)
    peak = (s + n).abs().amax(dim=1)

    def wave():
        return dict(ops.noise_aware_targets(s, n, lens, peak=peak, outputs=NAMES)[1])
    got = run_contract(monkeypatch, ops, wave)
    frames = [ops.target_frames(v)[1] for v in lens]
    _check_exact(got, _np_complex(ops.stft_complex(s)), _np_complex(ops.stft_complex(n)), "waveform", peak=peak.cpu().numpy(),
                 n_frames=frames)
    expect_refused(monkeypatch, ops, wave, "AVVAD_EINVAL", offset=1)            # the workspace 4 bytes off its alignment
    only = run_contract(monkeypatch, ops, lambda: dict(ops.noise_aware_targets(s, n, lens, peak=peak, outputs=("irm",))[1]))
    assert torch.equal(only["irm"], got["irm"])

    X, N = _spectra()
    Xd, Nd = torch.from_numpy(X).to(DEV), torch.from_numpy(N).to(DEV)
    got = run_contract(monkeypatch, ops, lambda: dict(ops.noise_aware_from_spectrum(Xd, Nd, n_frames=[3, 2], outputs=NAMES)),
                       short=None)                                              # (this entry point takes no workspace)
    _check_exact(got, X, N, "spectra", n_frames=[3, 2])
    got = run_contract(monkeypatch, ops, lambda: dict(ops.noise_aware_from_spectrum(Xd, None, outputs=("speech",))), short=None)
    _check_exact(got, X, None, "threshold")


def test_bad_arguments_are_refused_before_any_launch():
    """Through the C ABI: every refusal leaves the outputs and the workspace as they were; the proper calls succeed."""
    import numpy as np
    from avvad import _lib as L
    ops = _ops()
    lib = L.lib()
    lens, speech, noise = _ragged()
    s, n = torch.from_numpy(speech).to(DEV), torch.from_numpy(noise).to(DEV)
    B, Lp = s.shape
    T = 13
    tables = torch.zeros(2 * F + 1, dtype=torch.float64, device=DEV)           # room for the shift
    tables[:2 * F] = torch.from_numpy(np.concatenate(ops.noise_aware_tables(F))).to(DEV)
    cs, cn = tables[:F], tables[F:2 * F]
    off4 = lambda t: Ct.c_void_p(t.data_ptr() + 4)          # noqa: E731
    cnt = torch.tensor([lens, [ops.target_frames(v)[1] for v in lens]], dtype=torch.int32).to(DEV)
    outs = [torch.full((B, T, F), NAN, device=DEV) for _ in range(3)]
    d = L.TargetDesc(B, Lp, 1024, 256, T, 0, 0.0, 1.0, 1.0)
    nbytes = lib.avvad_target_noise_aware_workspace(Ct.byref(d))
    ws = torch.full((nbytes // 4 + 4,), NAN, device=DEV)

    def untouched(bufs):
        return all(bool(torch.isnan(t).all()) for t in bufs)

    def wave(s_p=L.ptr(s), n_p=L.ptr(n), frames_p=L.ptr(cnt[1]), cs_p=L.ptr(cs), cn_p=L.ptr(cn), low=5, high=500, out=outs,
             desc=d, ws_p=L.ptr(ws), ws_bytes=nbytes):
        return lib.avvad_target_noise_aware(s_p, n_p, L.ptr(cnt[0]), frames_p, None, cs_p, cn_p, low, high, 0.005,
                                            *[L.ptr(t) for t in out], Ct.byref(desc), ws_p, ws_bytes, _stream())
    centred = L.TargetDesc(B, Lp, 1024, 256, T, 1, 0.0, 1.0, 1.0)
    for rc, want in ((wave(ws_bytes=nbytes - 4), -2), (wave(cs_p=off4(cs)), -1), (wave(cn_p=off4(cn)), -1), (wave(ws_p=off4(ws)), -1),
                     (wave(out=[None] * 3), -1), (wave(low=0), -1), (wave(high=F + 1), -1), (wave(s_p=None), -1),
                     (wave(n_p=None), -1), (wave(frames_p=None), -1), (wave(cs_p=None), -1), (wave(ws_p=None), -1),
                     (wave(desc=centred), -1)):
        assert rc == want
        assert untouched(outs + [ws])
    assert wave() == 0
    want = ops.noise_aware_targets(s, n, lens, outputs=NAMES)[1]
    assert all(torch.equal(o, want[k]) for o, k in zip(outs, NAMES))
    assert bool(torch.isnan(ws[nbytes // 4:]).all())

    X = ops.stft_complex(s)                                                     # (B, T, F, 2)
    N = ops.stft_complex(n)
    for t in outs:
        t.fill_(NAN)
    st = X.stride()

    def spec(x_p=L.ptr(X), sx=st[:3], n_p=L.ptr(N), sn=st[:3], cs_p=L.ptr(cs), cn_p=L.ptr(cn), low=5, high=500, out=outs, shape=(B, T, F)):
        return lib.avvad_target_noise_aware_from_spectrum(x_p, *sx, n_p, *sn, L.ptr(cnt[1]), None, cs_p, cn_p, low, high, 0.005, 10.0,
                                                          *[L.ptr(t) for t in out], *shape, _stream())
    for rc in (spec(sx=(st[0], st[1], 3)), spec(sx=(st[0], st[1] + 1, 2)), spec(sx=(st[0] + 1, st[1], 2)), spec(sn=(st[0], st[1], 1)),
               spec(sx=(st[0], 0, 2)), spec(sx=(st[0], st[1], -2)), spec(sx=(0, st[1], 2)), spec(x_p=off4(X)), spec(n_p=off4(N)),
               spec(cs_p=off4(cs)), spec(cn_p=off4(cn)), spec(out=[None] * 3), spec(low=0), spec(high=F + 1), spec(x_p=None),
               spec(shape=(0, T, F)), spec(shape=(B, 0, F)), spec(shape=(B, T, 0))):
        assert rc == -1
        assert untouched(outs)
    assert spec() == 0
    assert all(torch.equal(o, want[k]) for o, k in zip(outs, NAMES))
    # a NULL noise spectrum is the constant noise power, whatever its strides say
    outs[0].fill_(NAN)
    assert spec(n_p=None, sn=(1, 1, 1), out=[outs[0], None, None]) == 0
    assert torch.equal(outs[0], ops.noise_aware_from_spectrum(X, None, n_frames=cnt[1], outputs=("speech",))["speech"])
