"""CPU tests of the masked inverse STFT: the C ABI's inventory and validation (no device needed: every call returns before
a launch), the host-side length rule, the oracle (tests/istft_ref.py) against scipy's independent ``istft``, and the
refusals of the Python layer."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
import torch

import istft_ref as R
from conftest import ROOT

NEW = ("avvad_istft_workspace", "avvad_istft", "avvad_resynth_workspace", "avvad_resynth", "avvad_stft_complex")
SHAPES = ((1024, 256, 12), (64, 16, 9), (96, 24, 7), (64, 48, 5))


def test_new_symbols_are_declared_bound_and_keep_the_abi_version():
    from avvad import _lib as L
    header = open(os.path.join(ROOT, "include", "avvad.h")).read()
    for name in NEW:
        assert name in L.SIGNATURES, name
        assert re.search(r"\b%s\(" % name, header), name
    assert "avvad_istft_desc" in header
    assert [n for n, _ in L.IstftDesc._fields_] == ["B", "T", "n_fft", "hop", "start", "out_pitch", "mask_mode"]
    assert L.ABI_VERSION == 3 and "#define AVVAD_ABI_VERSION 3" in header
    assert L.lib().avvad_abi_version() == 3


def test_workspace_queries_refuse_bad_descriptors():
    from avvad import _lib as L
    h = L.lib()
    ok = L.IstftDesc(3, 17, 1024, 256, 0, 5120, 1)
    sd = L.StftDesc(3, 5120, 1024, 256, 17, 0.0)
    need = h.avvad_istft_workspace(C.byref(ok))
    ld = 1028
    assert need >= (ld * 1024 + 3 * 17 * 1024) * 4 + 1024 * 8 + h.avvad_engine_workspace()      # Winv, Y, hann^2, engine scratch
    both = h.avvad_resynth_workspace(C.byref(sd), C.byref(ok))
    assert both >= need + (1024 * ld + 3 * 17 * ld) * 4                                           # + forward basis and spectrum
    bad = [L.IstftDesc(3, 17, 1024, 1025, 0, 5120, 1),       # hop > n_fft
           L.IstftDesc(3, 17, 1000, 250, 0, 5120, 1),        # n_fft % 32
           L.IstftDesc(3, 17, 16, 4, 0, 5120, 1),            # n_fft < 32
           L.IstftDesc(0, 17, 1024, 256, 0, 5120, 1),        # B = 0
           L.IstftDesc(3, 0, 1024, 256, 0, 5120, 1),
           L.IstftDesc(3, 17, 1024, 0, 0, 5120, 1),
           L.IstftDesc(3, 17, 1024, 256, 0, 0, 1),
           L.IstftDesc(3, 17, 1024, 256, -1, 5120, 1),
           L.IstftDesc(3, 17, 1024, 256, 0, 5120, 4),        # mask_mode outside 0..3
           L.IstftDesc(3, 17, 1024, 256, 0, 5120, -1)]
    p = 0x1000
    for d in bad:
        assert h.avvad_istft_workspace(C.byref(d)) == 0
        assert h.avvad_resynth_workspace(C.byref(sd), C.byref(d)) == 0
        assert h.avvad_istft(p, 17 * 1026, 1026, 2, p, None, None, None, p, C.byref(d), p, 1 << 40, None) == -1
        assert h.avvad_resynth(p, p, None, None, None, p, C.byref(sd), C.byref(d), p, 1 << 40, None) == -1
    assert h.avvad_istft_workspace(None) == 0 and h.avvad_resynth_workspace(None, C.byref(ok)) == 0
    # the two descriptors of a resynthesis must describe the same frames
    for other in (L.StftDesc(2, 5120, 1024, 256, 17, 0.0), L.StftDesc(3, 5120, 1024, 256, 16, 0.0),
                  L.StftDesc(3, 5120, 1024, 512, 9, 0.0), L.StftDesc(3, 5120, 1024, 256, 18, 0.0)):
        assert h.avvad_resynth_workspace(C.byref(other), C.byref(ok)) == 0
    # hop equal to n_fft and a hop that does not divide it are fine
    assert h.avvad_istft_workspace(C.byref(L.IstftDesc(1, 2, 64, 64, 0, 128, 0))) > 0
    assert h.avvad_istft_workspace(C.byref(L.IstftDesc(1, 5, 64, 48, 32, 100, 3))) > 0


def test_entry_points_validate_before_any_launch():
    from avvad import _lib as L
    h = L.lib()
    p = 0x1000                                                         # never dereferenced: every call below returns first
    d = L.IstftDesc(3, 17, 1024, 256, 0, 5120, 1)
    d0 = L.IstftDesc(3, 17, 1024, 256, 0, 5120, 0)
    sd = L.StftDesc(3, 5120, 1024, 256, 17, 0.0)
    need = h.avvad_istft_workspace(C.byref(d))
    st = (17 * 1026, 1026, 2)
    assert h.avvad_istft(None, *st, p, None, None, None, p, C.byref(d), p, need, None) == -1
    assert h.avvad_istft(p, *st, None, None, None, None, p, C.byref(d), p, need, None) == -1           # mode 1 needs a mask
    assert h.avvad_istft(p, *st, p, None, None, None, None, C.byref(d), p, need, None) == -1
    assert h.avvad_istft(p, *st, p, None, None, None, p, None, p, need, None) == -1
    assert h.avvad_istft(p, *st, p, None, None, None, p, C.byref(d), None, need, None) == -1
    assert h.avvad_istft(p, 0, 0, 2, p, None, None, None, p, C.byref(d), p, need, None) == -1           # frame stride 0
    assert h.avvad_istft(p, 0, 2, 0, p, None, None, None, p, C.byref(d), p, need, None) == -1
    assert h.avvad_istft(p, *st, p, None, None, None, p, C.byref(d), p, need - 1, None) == -2
    assert h.avvad_istft(p, *st, None, None, None, None, p, C.byref(d0), p, need - 1, None) == -2       # mode 0: NULL mask is fine
    both = h.avvad_resynth_workspace(C.byref(sd), C.byref(d))
    assert h.avvad_resynth(None, p, None, None, None, p, C.byref(sd), C.byref(d), p, both, None) == -1
    assert h.avvad_resynth(p, None, None, None, None, p, C.byref(sd), C.byref(d), p, both, None) == -1
    assert h.avvad_resynth(p, p, None, None, None, None, C.byref(sd), C.byref(d), p, both, None) == -1
    assert h.avvad_resynth(p, p, None, None, None, p, None, C.byref(d), p, both, None) == -1
    assert h.avvad_resynth(p, p, None, None, None, p, C.byref(sd), None, p, both, None) == -1
    assert h.avvad_resynth(p, p, None, None, None, p, C.byref(sd), C.byref(d), None, both, None) == -1
    assert h.avvad_resynth(p, p, None, None, None, p, C.byref(sd), C.byref(d), p, both - 1, None) == -2
    assert h.avvad_resynth(p, None, None, None, None, p, C.byref(sd), C.byref(d0), p, both - 1, None) == -2
    base = h.avvad_stft_workspace(C.byref(sd))
    assert h.avvad_stft_complex(None, p, C.byref(sd), p, base, None) == -1
    assert h.avvad_stft_complex(p, None, C.byref(sd), p, base, None) == -1
    assert h.avvad_stft_complex(p, p, None, p, base, None) == -1
    assert h.avvad_stft_complex(p, p, C.byref(sd), None, base, None) == -1
    assert h.avvad_stft_complex(p, p, C.byref(L.StftDesc(3, 5120, 1000, 250, 17, 0.0)), p, 1 << 40, None) == -1
    assert h.avvad_stft_complex(p, p, C.byref(sd), p, base - 1, None) == -2


def test_istft_length_against_the_oracle():
    from avvad import ops
    rng = np.random.default_rng(5)
    for n_fft, hop, T in SHAPES + ((64, 64, 3), (64, 16, 1)):
        S = R.random_spectrum(rng, T, n_fft)
        for center in (False, True):
            want = R.istft64(S, n_fft, hop, center=center)[0].size
            assert ops.istft_length(T, n_fft, hop, center) == want == R.istft_length(T, n_fft, hop, center)
    assert ops.istft_length(17, 1024, 256) == 5120 and ops.istft_length(17, 1024, 256, center=True) == 4096
    assert ops.istft_length(0, 1024, 256) == 0


@pytest.mark.parametrize("n_fft,hop,T", SHAPES)
def test_oracle_equals_scipy_istft(n_fft, hop, T):
    """scipy.signal.istft(S / hann.sum(), boundary=False) is the same transform with a 1e-10 threshold on the window sum of
    squares: wherever that holds the two agree to float64 rounding; at most 3 samples per utterance fall below it (1024 /
    256: samples 0, 1 and the last; the small shapes: sample 0).  Inputs have unit-peak frames, so differences are taken
    relative to max(|y|, 1)."""
    from scipy import signal
    S = R.random_spectrum(np.random.default_rng(n_fft + hop), T, n_fft).astype(np.complex128)
    y, num, wss = R.istft64(S, n_fft, hop)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # scipy notes that hop 48 of 64 fails its NOLA test at sample 0
        _, x = signal.istft((S / R.hann(n_fft).sum()).T, fs=1.0, window="hann", nperseg=n_fft, noverlap=n_fft - hop, nfft=n_fft,
                            boundary=False)
    assert x.shape == y.shape == (n_fft + hop * (T - 1),)
    ok = wss > 1e-10
    left_out = np.flatnonzero(~ok).tolist()
    assert left_out == ([0, 1, y.size - 1] if (n_fft, hop) == (1024, 256) else [0]), left_out
    rel = float((np.abs(x - y)[ok] / np.maximum(np.abs(y[ok]), 1.0)).max())
    print("oracle vs scipy %d/%d: max relative difference %.2e over %d samples" % (n_fft, hop, rel, int(ok.sum())))
    assert rel <= 1e-13
    # the numerator and the float32 GEMM form are the same transform
    e32 = R.weighted_error(R.istft32_gemm(S, n_fft, hop), num, wss)[0]
    print("float32 GEMM form %d/%d: E_cpu32 = %.2e" % (n_fft, hop, e32))
    assert 0 < e32 < 5e-6


def test_host_tensors_are_refused():
    from avvad import ops
    from avvad._lib import AvvadError
    from packages.processing.stft import istft
    S = torch.from_numpy(R.random_spectrum(np.random.default_rng(1), 5, 64))          # (T, F) complex64 on the host
    with pytest.raises(AvvadError, match="GPU"):
        istft(S.T, fs=16000, wlen_sec=64 / 16000)
    with pytest.raises(AvvadError, match="GPU"):
        istft(torch.view_as_real(S.T.contiguous()), fs=16000, wlen_sec=64 / 16000)
    with pytest.raises(ValueError, match="integer"):
        istft(S.T, fs=16000, wlen_sec=64.5 / 16000)
    with pytest.raises(AvvadError, match="GPU"):
        ops.istft(S.T, 64, 16)
    with pytest.raises(AvvadError, match="GPU"):
        ops.istft(torch.view_as_real(S)[None], 64, 16)
    with pytest.raises(AvvadError, match="GPU"):
        ops.stft_complex(torch.zeros(2, 4000), 64, 16)
    with pytest.raises(AvvadError, match="GPU"):
        ops.resynth(torch.zeros(2, 4000), None, mask_mode=0)


def test_evaluator_refuses_resynthesis_without_a_mask_model(tmp_path):
    """checked before the device is set up: a y_dim = 1 model, another network kind, no wav_list"""
    from avvad import train as TR
    from packages.models.Audio_Net import DeepVAD_audio
    with pytest.raises(ValueError, match="513"):
        TR.evaluate_main("audio", lambda: DeepVAD_audio(1, 8, 1), wav_list=[], out_dir=str(tmp_path / "o"),
                         resynth_dir=str(tmp_path / "r"))
    with pytest.raises(ValueError, match="resynth_dir"):
        TR.evaluate_main("audio", lambda: DeepVAD_audio(1, 8, 513), out_dir=str(tmp_path / "o"), resynth_dir=str(tmp_path / "r"))
    with pytest.raises(ValueError, match="resynth_dir"):
        TR.evaluate_main("video", lambda: None, wav_list=[], out_dir=str(tmp_path / "o"), resynth_dir=str(tmp_path / "r"))
    assert not os.path.exists(str(tmp_path / "o")) and not os.path.exists(str(tmp_path / "r"))
    with pytest.raises(ValueError, match="513"):
        TR.resynth_utt(DeepVAD_audio(1, 8, 1), torch.zeros(4000))
