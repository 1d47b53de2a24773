"""CPU tests of the training labels (packages/processing/target.py): the float64 restatement (tests/target_ref.py) against
the reference's own float32 results (tests/golden/targets.npz), the C ABI's descriptor validation, and the drop-in's
refusal to run without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import target_ref as R
from conftest import GOLDEN, load_golden

CFGS = {"c64f": dict(wlen_sec=64e-3, center=False), "c64t": dict(wlen_sec=64e-3, center=True), "d50": dict()}

# VAD band: the reference sums 1024 float32 squares in sequence, relative error <= n u = 1024 * 2^-24 ~ 6e-5 of E, so a
# frame whose float64 energy lies within 1e-4 of the threshold may fall either way.
VAD_BAND = 1e-4
# IBM band: every bin is a 1024-term float32 dot product (torch.stft on the reference's side, an fp32 MFMA GEMM on the
# GPU).  Its rounding error is ~ sqrt(n) u |frame| in practice -- measured 1e-7 of max|S| for torch.stft on sa1 against a
# float64 DFT -- so bins whose float64 magnitude lies within DELTA = 2e-6 of max|S| (20x that) of the threshold
# magnitude may fall either way.  The reference's float32 log10 adds ~1e-9 of max|S| at the threshold, far inside.
IBM_DELTA = 2e-6


def sa1(tag):
    x = np.load("%s/%s.npz" % (GOLDEN, "utt_sa1_clean" if tag == "clean" else "utt_sa1"))["samples"].astype(np.float32) / 32768.0
    return x / np.max(np.abs(x))


def vad_band(E, c):
    thr = c * E.min()
    return np.abs(E - thr) <= VAD_BAND * thr


def ibm_band(mag, M, tau):
    return np.abs(mag - tau) <= IBM_DELTA * M


def ref_spectrum(x):
    from oracle import frontend
    return torch.view_as_complex(frontend.stft(torch.from_numpy(x), wlen_sec=64e-3, center=False)).numpy()


@pytest.mark.parametrize("tag", ["clean", "noisy"])
@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_restated_vad_matches_reference(tag, cfg):
    g = load_golden("targets")
    E, c = R.vad_energy(sa1(tag), **CFGS[cfg])
    ours = R.clean_speech_VAD(sa1(tag), **CFGS[cfg])[0].astype(bool)
    ref = g["vad_%s_%s" % (tag, cfg)][0].astype(bool)
    band = vad_band(E, c)
    print("VAD %s %s: %d frames, %d in the band" % (tag, cfg, len(E), band.sum()))
    assert ours.shape == ref.shape
    assert band.sum() <= 2
    assert np.array_equal(ours[~band], ref[~band])


@pytest.mark.parametrize("thr", [50, 65])
def test_restated_ibm_matches_reference(thr):
    g = load_golden("targets")
    S = ref_spectrum(sa1("clean"))
    mask, mag, M, tau = R.ibm_parts(S, 1e-8, thr)
    ref = g["ibm%d_clean" % thr].astype(bool)
    band = ibm_band(mag, M, tau)
    print("IBM thr %d: %d bins, %d in the band" % (thr, mask.size, band.sum()))
    assert mask.shape == ref.shape == (513, 185)
    assert band.sum() <= 0.002 * mask.size
    assert np.array_equal(mask[~band], ref[~band])
    if thr == 50:
        robust = R.noise_robust_clean_speech_IBM(sa1("clean"), S, wlen_sec=64e-3, center=False).astype(bool)
        E, c = R.vad_energy(sa1("clean"), wlen_sec=64e-3, center=False)
        ok = ~band & ~vad_band(E, c)[None, :]
        assert np.array_equal(robust[ok], g["robust_clean"].astype(bool)[ok])


def test_restated_edge_cases_match_reference():
    g = load_golden("targets")
    for name in ("silence", "zeros", "whole", "one"):
        x = g["edge_%s" % name]
        ours = R.clean_speech_VAD(x, wlen_sec=64e-3, center=False)
        assert np.array_equal(ours.astype(np.uint8), g["edge_vad_%s" % name]), name
    assert g["edge_vad_one"].shape == (1, 1) and g["edge_vad_whole"].shape == (1, 27)     # 7680 = 30 hops: no end pad
    E, _ = R.vad_energy(g["edge_silence"], wlen_sec=64e-3, center=False)
    assert E.min() == 0.0 and np.array_equal(g["edge_vad_silence"][0].astype(bool), E > 0)  # min E = 0 -> vad = E > 0
    assert g["edge_ibm_zeros"].all() and not g["edge_vad_zeros"].any()        # all-zero: IBM all ones, VAD all zeros


def test_target_workspace_rejects_bad_descriptors():
    from avvad import _lib as L
    h = L.lib()

    def ws(B=2, Lp=48100, n_fft=1024, hop=256, T=185, center=0):       # sa1's 48100 samples: 185 frames, 189 centred
        return h.avvad_target_workspace(C.byref(L.TargetDesc(B, Lp, n_fft, hop, T, center, 1e-8, 10 ** 1.7, 10 ** -2.5)))
    assert ws() > 0
    assert ws(T=1) > 0 and ws(center=1, T=189) > 0 and ws(center=2, T=189) > 0
    assert ws(B=0) == 0
    assert ws(hop=0) == 0 and ws(hop=-256) == 0
    assert ws(T=186) == 0                       # (T-1) hop + n_fft > L + one hop of end pad
    assert ws(center=1, T=190) == 0
    assert ws(center=3) == 0 and ws(T=0) == 0 and ws(n_fft=0) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a GPU")
def test_drop_in_refuses_host_input_without_gpu():
    from avvad._lib import AvvadError
    from packages.processing import target
    x = sa1("clean")
    with pytest.raises(AvvadError):
        target.clean_speech_VAD(x)
    with pytest.raises(AvvadError):
        target.clean_speech_IBM(np.ones((513, 4), np.complex64))
    with pytest.raises(AvvadError):
        target.noise_robust_clean_speech_IBM(x, np.ones((513, 4), np.complex64))
