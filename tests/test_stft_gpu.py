"""The whole-utterance STFT front-end (csrc/stft.hip behind ``ops.stft`` / ``ops.stft_complex`` and the drop-ins of
``packages.processing.stft``) on the MI355X against tests/stft_ref.py: every case of its three tiers through the HIP path,
with nothing here but calls into its assertion functions, the refusals and the run-to-run reproducibility."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import stft_ref as R
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu


def _workspace_spectrum(w, cfg):
    """avvad_stft_complex on a NaN-filled workspace of its own -> the workspace's [M][ld] spectrum"""
    from avvad import _lib as L
    from avvad import ops
    B, Ls = w.shape
    N, hop = cfg["n_fft"], cfg["hop"]
    T = ops.n_frames(Ls, N, hop, cfg["pad"], cfg["fs"])
    d = L.StftDesc(B, Ls, N, hop, T, 0.0)
    nbytes = L.lib().avvad_stft_workspace(Ct.byref(d))
    assert nbytes > 0
    ws = torch.full(((nbytes + 3) // 4,), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.empty((B, T, N // 2 + 1, 2), dtype=torch.float32, device=DEV)
    stream = Ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lib().avvad_stft_complex(L.ptr(w), L.ptr(out), Ct.byref(d), L.ptr(ws), nbytes, stream)
    assert rc == 0
    torch.cuda.synchronize()
    ld, s0 = R.spectrum_ld(N), R.ws_spectrum_offset(N)
    return ws[s0:s0 + B * T * ld].view(B * T, ld)


def hip_impl(what, wave, cfg):
    from avvad import ops
    from packages.processing import stft as P
    N, hop, fs = cfg["n_fft"], cfg["hop"], cfg["fs"]
    w = torch.from_numpy(np.array(wave, dtype=np.float32)).to(DEV)         # (a copy: the cached signals are read-only)
    kw = dict(n_fft=N, hop=hop, pad_at_end=cfg["pad"], fs=fs)
    if what == "complex":
        out = ops.stft_complex(w, **kw)
    elif what == "legacy":
        out = ops.stft(w[0], mode=2, **kw)
    elif what == "power":
        out = ops.stft(w, mode=1, eps=cfg["eps"], **kw)
    elif what == "log":
        out = ops.stft(w, mode=0, eps=cfg["eps"], **kw)
    elif what == "std":
        out = ops.stft(w, mode=0, eps=cfg["eps"], mean=torch.from_numpy(cfg["mean"]).to(DEV), std=torch.from_numpy(cfg["std"]).to(DEV),
                       norm_eps=cfg["norm_eps"], **kw)
    elif what == "workspace":
        out = _workspace_spectrum(w, cfg)
    elif what == "center":
        out = P.stft_pytorch(w[0], fs=fs, wlen_sec=N / fs, hop_percent=hop / N, center=True, pad_at_end=cfg["pad"])
    else:
        assert what == "lps" and int((N / fs) * fs) == N and int((hop / N) * N) == hop
        out = P.log_power_spectrogram(w, fs=fs, wlen_sec=N / fs, hop_percent=hop / N, eps=cfg["eps"], pad_at_end=cfg["pad"])
    return out.cpu().numpy()


IMPULSE_COUNT = [0, 0]


@pytest.mark.parametrize("name", R.IMPULSE)
def test_impulse_tier(name):
    off, total = R.check_impulse(hip_impl, name)
    IMPULSE_COUNT[0] += off
    IMPULSE_COUNT[1] += total


def test_log_the_impulse_tier_count():
    R.H.log_line("stft gpu          impulse tier: %d of %d non-zero elements one ulp off float32(reference)" % tuple(IMPULSE_COUNT))


@pytest.mark.parametrize("name", R.ROUNDING)
def test_rounding_tier(name):
    fig = R.check_rounding(hip_impl, name)
    assert fig["worst"] > 0
    if R.CASES[name]["features"]:
        R.check_features(hip_impl, name)


@pytest.mark.parametrize("name", R.SILENCE)
def test_silence(name):
    R.check_silence(hip_impl, name)


@pytest.mark.parametrize("name", R.CENTER)
def test_centred_wrapper(name):
    R.check_center(hip_impl, name)


def test_the_schedule_case_is_bit_identical_run_to_run():
    from avvad import ops
    c = R.CASES[R.SCHEDULE_CASE]
    w = torch.from_numpy(np.array(R.signal(R.SCHEDULE_CASE))).to(DEV)
    a = ops.stft_complex(w, c["n_fft"], c["hop"], c["pad"], c["fs"])
    b = ops.stft_complex(w, c["n_fft"], c["hop"], c["pad"], c["fs"])
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    la, lb = ops.stft(w, c["n_fft"], c["hop"], mode=0), ops.stft(w, c["n_fft"], c["hop"], mode=0)
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32))


def test_refusals_before_any_launch():
    """a wave shorter than n_fft that one hop of padding does not help, mode 2 with two utterances, a mean without a std,
    n_fft = 48: AvvadError"""
    from avvad import ops
    from avvad._lib import AvvadError
    w = torch.zeros(2, 16000, device=DEV)
    for call in (lambda: ops.stft(torch.zeros(700, device=DEV)),
                 lambda: ops.stft_complex(torch.zeros(700, device=DEV)),
                 lambda: ops.stft(torch.zeros(1000, device=DEV), pad_at_end=False),
                 lambda: ops.stft(w, mode=2),
                 lambda: ops.stft(w, mean=torch.zeros(513, device=DEV)),
                 lambda: ops.stft(w, mode=1, mean=torch.zeros(513, device=DEV), std=torch.ones(513, device=DEV)),
                 lambda: ops.stft(w, n_fft=48, hop=16),
                 lambda: ops.stft_complex(w, n_fft=48, hop=16)):
        with pytest.raises(AvvadError):
            call()
    assert ops.stft(torch.zeros(1000, device=DEV)).shape == (1, 1, 513)        # one hop of padding helps here
