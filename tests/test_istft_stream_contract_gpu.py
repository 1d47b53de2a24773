"""The caller-owned buffer contract of include/avvad.h for the streaming inverse STFT family (avvad_stft_stream_fwd_spec,
avvad_istft_stream_basis, avvad_istft_stream), through tests/abi_guard.py as tests/test_abi_contract_gpu.py does for the
other families: zero-, NaN- and 1e30-filled guarded workspace, outputs and spare states give the same bits with the guards
intact; a workspace one float short is refused (AVVAD_EWORKSPACE) with everything still poisoned; a workspace or a basis
4 bytes off its 16-byte alignment is refused (AVVAD_EINVAL) before anything is launched."""
import ctypes as Ct

import numpy as np
import pytest
import torch

from abi_guard import expect_refused, run_contract
from test_istft_gpu import _check_row

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
T_ = torch.from_numpy


def _ops():
    from avvad import ops
    return ops


def _stream():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_samples_in_samples_out_with_poisoned_buffers(monkeypatch):
    """Two rows of 3000 and 2100 samples in two packets through stft_stream(return_spec=True) and istft_stream with a
    given mask: both bases, the features, the spectrum, the samples and both spare states are outputs and poisoned, the
    inverse's workspace is guarded.  The samples go against the oracle of the float64-masked spectrum the test computes."""
    from avvad.stream import OlaClock, SampleClock
    ops = _ops()
    n_fft, hop, lens = 1024, 256, [3000, 2100]
    rng = np.random.default_rng(5)
    x = np.zeros((2, 3000), dtype=np.float32)
    for b, n in enumerate(lens):
        v = rng.standard_normal(n)
        x[b, :n] = v / np.abs(v).max()
    xd = T_(x).to(DEV)
    T = [ops.n_frames(n, n_fft, hop) for n in lens]
    mask = rng.random((2, max(T), 513)).astype(np.float32)
    md = T_(mask).to(DEV)

    def case():
        fb, ib = ops.stft_stream_basis(n_fft, DEV), ops.istft_stream_basis(n_fft, DEV)
        sc, oc = SampleClock(2, n_fft, hop), OlaClock(2, n_fft, hop)
        fs, os_ = ops.stft_stream_state(2, n_fft, DEV), ops.istft_stream_state(2, n_fft, DEV)
        fspare, ospare = ops.torch.empty_like(fs), ops.torch.empty_like(os_)
        outs, specs, done = [[], []], [[], []], [0, 0]
        for s0, s1 in ((0, 1700), (1700, 3000)):
            n = [min(max(l - s0, 0), s1 - s0) for l in lens]
            fin = [b for b in range(2) if s0 < lens[b] <= s1]
            f, frames, spec = ops.stft_stream(xd[:, s0:s1].contiguous(), n, sc, fs, fb, final=fin, out_state=fspare, return_spec=True)
            fs, fspare = fspare, fs
            m = torch.full((2, max(frames), 513), NAN, device=DEV)
            for b in range(2):
                m[b, :frames[b]] = md[b, done[b]:done[b] + frames[b]]
            y, n_out = ops.istft_stream(spec, frames, oc, os_, ib, mask=m, final_samples={b: lens[b] for b in fin}, out_state=ospare)
            os_, ospare = ospare, os_
            for b in range(2):
                outs[b].append(y[b, :n_out[b]])
                specs[b].append(spec[b, :frames[b]])
                done[b] += frames[b]
        assert done == T and oc.written == lens
        return {"y0": torch.cat(outs[0]), "y1": torch.cat(outs[1]), "spec0": torch.cat(specs[0]), "spec1": torch.cat(specs[1]),
                "state": os_, "front": fs, "basis": ib.view(torch.int32)}         # (hann^2 sits in it as doubles: compared as bits)

    ib0 = ops.istft_stream_basis(n_fft, DEV)
    spec0 = torch.randn(2, 3, 513, 2, device=DEV)

    def inverse_alone():
        oc = OlaClock(2, n_fft, hop)
        return ops.istft_stream(spec0, [3, 2], oc, ops.istft_stream_state(2, n_fft, DEV), ib0, mask=md[:, :3].contiguous(),
                                out_state=ops.torch.empty(2, n_fft, dtype=torch.float32, device=DEV))
    got = run_contract(monkeypatch, ops, case, short_ops={"avvad_istft_stream": inverse_alone})
    assert torch.count_nonzero(got["state"]).item() == 0
    for b, n in enumerate(lens):
        assert got["y%d" % b].shape == (n,)
        S = got["spec%d" % b].cpu().numpy().astype(np.float64)
        S64 = (S[..., 0] + 1j * S[..., 1]) * mask[b, :T[b]].astype(np.float64)
        _check_row("contract: stream row %d" % b, got["y%d" % b], S64, n_fft, hop, length=n)
    # the workspace 4 bytes off its alignment
    expect_refused(monkeypatch, ops, inverse_alone, "AVVAD_EINVAL", offset=1)


def test_misaligned_bases_are_refused():
    """Through the C ABI with a pointer 4 bytes off: building the inverse basis, using it, and the forward basis of
    avvad_stft_stream_fwd_spec return AVVAD_EINVAL, and the outputs keep their contents."""
    from avvad import _lib as L
    from avvad.stream import SampleClock
    ops = _ops()
    lib = L.lib()
    off4 = lambda t: Ct.c_void_p(t.data_ptr() + 4)      # noqa: E731
    n_fft, hop = 64, 16
    nb = lib.avvad_istft_stream_basis_bytes(n_fft) // 4
    bbuf = torch.full((nb + 4,), NAN, device=DEV)
    assert lib.avvad_istft_stream_basis(n_fft, off4(bbuf), _stream()) == -1 and bool(torch.isnan(bbuf).all())
    basis = ops.istft_stream_basis(n_fft, DEV)
    bbuf[1:1 + nb].copy_(basis)
    spec = torch.randn(1, 3, 33, 2, device=DEV)
    counts = torch.tensor([[3], [0], [48]], dtype=torch.int32, device=DEV)
    state, new = torch.zeros(1, n_fft, device=DEV), torch.full((1, n_fft), NAN, device=DEV)
    out = torch.full((1, 48), NAN, device=DEV)
    d = L.IstftStreamDesc(1, 3, n_fft, hop, 48, 3, 0)
    ws = torch.full(((lib.avvad_istft_stream_workspace(Ct.byref(d)) + 3) // 4 + 4,), NAN, device=DEV)
    args = lambda b, w: (L.ptr(spec), None, L.ptr(counts[0]), L.ptr(counts[1]), L.ptr(counts[2]), None, L.ptr(state), L.ptr(new),      # noqa: E731
                         b, L.ptr(out), Ct.byref(d), w, (ws.numel() - 4) * 4, _stream())
    for b, w in ((off4(bbuf), L.ptr(ws)), (L.ptr(basis), off4(ws))):
        assert lib.avvad_istft_stream(*args(b, w)) == -1
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(new).all()) and bool(torch.isnan(ws).all())
    assert lib.avvad_istft_stream(*args(L.ptr(basis), L.ptr(ws))) == 0
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(new).all())
    S = spec[0].cpu().numpy().astype(np.float64)
    _check_row("contract: direct call", out[0], S[..., 0] + 1j * S[..., 1], n_fft, hop, length=48)
    # avvad_stft_stream_fwd_spec's basis
    n_fft, hop = 1024, 256
    nb = lib.avvad_stft_stream_basis_bytes(n_fft) // 4
    fbuf = torch.full((nb + 4,), NAN, device=DEV)
    fbasis = ops.stft_stream_basis(n_fft, DEV)
    fbuf[1:1 + nb].copy_(fbasis)
    chunk = torch.randn(1, 2048, device=DEV)
    frames, pending, pad = SampleClock(1, n_fft, hop).advance([2048])
    assert frames == [5]
    counts = torch.tensor([[2048], pending, frames, pad], dtype=torch.int32, device=DEV)
    state, new = torch.zeros(1, n_fft, device=DEV), torch.full((1, n_fft), NAN, device=DEV)
    feat, sp = torch.full((1, 5, 513), NAN, device=DEV), torch.full((1, 5, 513, 2), NAN, device=DEV)
    sd = L.StftStreamDesc(1, 2048, n_fft, hop, 5, 5, 1e-8, 1e-8)
    fargs = lambda b: (L.ptr(chunk), L.ptr(counts[0]), L.ptr(counts[1]), L.ptr(counts[2]), L.ptr(counts[3]), None, L.ptr(state),      # noqa: E731
                       L.ptr(new), b, None, None, L.ptr(feat), L.ptr(sp), Ct.byref(sd), _stream())
    assert lib.avvad_stft_stream_fwd_spec(*fargs(off4(fbuf))) == -1
    assert bool(torch.isnan(feat).all()) and bool(torch.isnan(sp).all()) and bool(torch.isnan(new).all())
    assert lib.avvad_stft_stream_fwd_spec(*fargs(L.ptr(fbasis))) == 0
    assert bool(torch.isfinite(feat).all()) and bool(torch.isfinite(sp).all())
