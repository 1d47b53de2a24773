"""CPU tests of the training labels (packages/processing/target.py): the float64 restatement (tests/target_ref.py) against
the reference's own float32 results (tests/golden/targets.npz), the C ABI's descriptor validation, the drop-in's
refusal to run without a GPU, and the conditions under which the cases of tests/target_ref.py that are aimed at the
launch shapes of csrc/target.hip can fail on the GPU (the constants read back from the source, ones shares, empty tie
bands, and the labels that a minimum or maximum lost between loop trips would change)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import target_ref as R
from conftest import GOLDEN, PKG, load_golden

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


# ------------------------------------------------------------------ the cases aimed at target.hip's launch shapes
# Each condition below is asserted from the float64 reference alone: it is what makes the GPU test of the same case
# (tests/test_targets_gpu.py, tests/test_noise_aware_gpu.py) able to fail.
TIE = 1e-12          # the VAD tie band of test_targets_gpu.py


def test_case_constants_match_the_source():
    """the launch constants the case builders of target_ref aim with, read back from csrc/target.hip"""
    with open(os.path.join(PKG, "csrc", "target.hip")) as f:
        src = f.read()
    assert int(re.search(r"constexpr int SEGS_PER_WAVE = (\d+);", src).group(1)) == R.SEGS_PER_WAVE
    assert int(re.search(r"constexpr int MAX_ROWS = (\d+);", src).group(1)) == R.MAX_ROWS
    kernels = re.findall(r"__global__ void __launch_bounds__\((\d+)\)\s+(\w+)\(", src)
    assert sorted(k for _, k in kernels) == sorted(["segment_energy", "vad_decide", "spectrum_max", "ibm_mask", "spectrum_max_strided",
                                                    "ibm_mask_strided", "noise_aware_mask"])
    assert all(int(n) == R.WG for n, _ in kernels)
    assert src.count("dim3(256)") == len(kernels) == 7          # one launch each, all of 256 threads
    caps = {k: int(c) for k, c in re.findall(r"hipLaunchKernelGGL\((\w+), dim3\(grid_cap\(n4(?: \* 4)?, (\d+)\)\)", src)}
    assert caps == dict(ibm_mask=R.CAP_MASK, noise_aware_mask=R.CAP_MASK, ibm_mask_strided=R.CAP_MASK_STRIDED,
                        spectrum_max_strided=R.CAP_MAX_STRIDED)
    assert "dim3(grid_cap(n4 * 4, 1024))" in src                # the maximum pass: one bin per thread
    # the strides the trip counts follow from
    assert "for (int t = tid; t < T; t += 256) mn = fmin(" in src and "for (int t4 = tid * 4; t4 < Tp; t4 += 1024)" in src
    assert "for (int t = tid; t < Tp; t += 256) out[t]" in src and "for (int k = lane * 4; k < seg; k += 256)" in src
    assert "(int)(aligned16(vad) && d->T % 4 == 0)" in src and "const int vec = aligned16(wave) && d->L % 4 == 0;" in src
    assert "return d->n_fft % d->hop == 0 ? d->n_fft / d->hop : 1;" in src and "const int seg = R > 1 ? d->hop : d->n_fft;" in src
    assert (R.MASK_TRIP, R.MASK_STRIDED_TRIP, R.MAX_STRIDED_TRIP) == (8388608, 4194304, 262144)


@pytest.mark.parametrize("name", sorted(R.vad_cases()))
def test_vad_cases_reach_what_they_aim_at(name):
    from avvad import ops
    case = R.vad_cases()[name]
    n_fft, hop = case["n_fft"], case["hop"]
    kw = R.framing(n_fft, hop)
    assert int(kw["wlen_sec"] * kw["fs"]) == n_fft == kw["wlen_sec"] * kw["fs"] and int(kw["hop_percent"] * n_fft) == hop
    for mode in case.get("center") or (None,):
        for b, x in enumerate(case["rows"]):
            E, c = R.vad_reference(case, b, mode)
            T = ops.target_frames(len(x), center=mode is not None, **kw)[1]
            assert len(E) == T == case["T"][b]
            thr = c * E.min()
            ones = (E > thr).mean()
            print("%s %s row %d: T %d, %.1f %% ones, quietest frame %d" % (name, mode, b, T, 100 * ones, E.argmin()))
            assert E.min() > 0 and not (np.abs(E - thr) <= TIE * thr).any()
            assert 0.10 <= ones <= 0.90

    def labels(E):
        return E > c * E.min()

    def flips(E_wrong, E_right, what, least=5):
        n = int((labels(E_wrong) != labels(E_right)).sum())
        print("%s: %s changes %d labels" % (name, what, n))
        assert n >= least, (name, what, n)
    E0, c = R.vad_reference(case, 0, "reflect" if case.get("center") else None)
    if name in R.LATE_MIN:
        assert R.LATE_MIN[name] == 0 and len(E0) > 1024 and E0.argmin() >= 768
        n = int((labels(E0) != (E0 > c * E0[:256].min())).sum())
        print("%s: the minimum of the first 256 frames alone changes %d labels" % (name, n))
        assert n >= 5
    if name == "scalar_store_T1027":
        assert len(E0) % 4 and E0.argmin() >= len(E0) - 4
        assert labels(E0)[1024:].tolist() == [True, True, False]      # the store loop's fifth trip writes both labels
    if name == "vec_store_T1028":
        assert len(E0) % 4 == 0
    if not case.get("center") and name not in R.LATE_MIN:
        # the cases aimed at segment_energy: the model without a mistake is the reference, each mistake changes labels
        assert np.allclose(R.segment_model(case), E0, rtol=1e-12, atol=0)
        seg = n_fft if n_fft % hop else hop
        k = np.arange(seg)
    if name.startswith("whole_frame"):
        assert n_fft % hop and n_fft == 4 * R.WG and hop % 4 and (len(case["rows"][0]) % 4 == 0) == (name == "whole_frame_vec")
        for trips in (1, 2, 3):
            flips(R.segment_model(case, keep=k < trips * R.WG), E0, "keeping %d of the four k trips" % trips)
        if name == "whole_frame_vec":
            flips(R.segment_model(case, aligned=True), E0, "taking every float4 load from an aligned address")
    if name.startswith("ragged_quad"):
        assert seg % 4 == 2
        flips(R.segment_model(case, keep=k < seg - 2), E0, "dropping the last quad's two samples")
        flips(R.segment_model(case, keep=k < seg - 1), E0, "dropping the last sample", least=2)
        flips(R.segment_model(case, over=2), E0, "an unguarded last quad")
        flips(R.segment_model(case, over=1), E0, "a last quad guarded one sample late", least=2)
    if name == "hop_block_seg512":
        assert n_fft % hop == 0 and hop == 2 * R.WG
        flips(R.segment_model(case, keep=k < R.WG), E0, "dropping the second k trip")
        flips(R.segment_model(case, keep=k >= R.WG), E0, "dropping the first k trip")
    if name == "centred_ragged":
        lens = [len(x) for x in case["rows"]]
        pads = [ops.target_frames(n, **kw)[0] - n for n in lens]
        assert lens[0] == max(lens) and pads == [hop, 0, hop] and min(lens) > n_fft // 2
        for b in range(len(lens)):
            Er, _ = R.vad_reference(case, b, "reflect")
            Ec, _ = R.vad_reference(case, b, "constant")
            assert np.allclose(R.centred_model(case, b, "reflect"), Er, rtol=1e-12, atol=0)
            assert np.allclose(R.centred_model(case, b, "constant"), Ec, rtol=1e-12, atol=0)
            flips(Ec, Er, "row %d: 'constant' in the place of 'reflect'" % b, least=1)
            if pads[b]:
                flips(R.centred_model(case, b, "reflect", reflect_at="length"), Er, "row %d: reflecting about the length without "
                      "the end pad" % b, least=1)
            if b:
                flips(R.centred_model(case, b, "reflect", reflect_at="widest"), Er, "row %d: reflecting about the widest row's "
                      "end" % b, least=1)
        for mode in case["center"]:
            flips(R.centred_model(case, 0, mode, bounded=False), R.centred_model(case, 0, mode), "row 0, %s: reading the end pad "
                  "behind the batch's width" % mode, least=1)
    if name == "long_and_short":
        E1, _ = R.vad_reference(case, 1)
        assert len(E1) < 256 and 1e3 <= np.median(E1) / np.median(E0) <= 1e5      # 100x in level: 1e4 in energy


@functools.lru_cache(maxsize=1)
def ibm_case():
    """the waveform IBM batch and, per row, the float64 spectrum (T_b, 513), the mask and the band: computed once"""
    import noise_aware_ref as NA
    rows = R.ibm_rows()
    ref = []
    for x in rows:
        S = NA.dft64(x)
        mask, mag, M, tau = R.ibm_parts(S)
        E, c = R.vad_energy(x, wlen_sec=64e-3, center=False)
        band = ibm_band(mag, M, tau)
        full = len(S) - len(S) % R.MAX_ROWS                   # what a maximum over the whole slabs alone would decide
        lost = int(((mag > (mag[:full].max() + 1e-8) * 10.0 ** -2.5 - 1e-8) != mask)[~band].sum())
        ref.append(dict(mask=mask, band=band, peak_frame=int(np.unravel_index(mag.argmax(), mag.shape)[0]), M=M, E=E,
                        vad_thr=c * E.min(), lost=lost))
    return rows, ref


def test_ibm_batch_reaches_what_it_aims_at():
    from avvad import ops
    rows, ref = ibm_case()
    T = [r["mask"].shape[0] for r in ref]
    assert T == list(R.IBM_FRAMES) == [ops.target_frames(len(x))[1] for x in rows] and T[-1] == max(T) and T[-1] % 2
    assert all(t % R.MAX_ROWS for t in T)
    n = len(T) * max(T) * 513
    assert R.trips(n, R.MASK_TRIP) == 2
    for b, r in enumerate(ref):
        ones, share = r["mask"].mean(), r["band"].mean()
        print("IBM row %d: T %d, max|S| %.3g in frame %d, %.1f %% ones, %.2e of the bins in the band"
              % (b, T[b], r["M"], r["peak_frame"], 100 * ones, share))
        assert 0.10 <= ones <= 0.90 and share <= 0.002
        assert len(r["E"]) == T[b] and r["E"].min() > 0 and not (np.abs(r["E"] - r["vad_thr"]) <= TIE * r["vad_thr"]).any()
        assert 0.05 <= (r["E"] > r["vad_thr"]).mean() <= 0.95          # the robust mask is neither the plain one nor empty
        if b in R.IBM_LATE_PEAK:
            print("IBM row %d: without its partial last slab the maximum changes %d labels outside the band" % (b, r["lost"]))
            assert r["peak_frame"] == T[b] - 1 and r["lost"] >= 1000
    M = sorted(r["M"] for r in ref)
    assert M[-1] / M[0] >= 1e3 and M[1] / M[0] >= 30                   # levels 100x apart
    # the second trip: the last outputs of the last row, live frames that hold both labels
    tail = ref[-1]["mask"].reshape(-1)[R.MASK_TRIP - n:]
    assert 0.05 <= tail.mean() <= 0.95


@functools.lru_cache(maxsize=1)
def spectrum_case():
    S, vad = R.strided_spectrum()
    mask, undecided = R.ibm_exact(S)
    return S, vad, mask, undecided


def test_strided_spectrum_reaches_what_it_aims_at():
    S, vad, mask, undecided = spectrum_case()
    n = S.size
    assert S.shape == (R.SPEC_F, R.SPEC_T) and R.trips(n, R.MAX_STRIDED_TRIP) == 17 and R.trips(n, R.MASK_STRIDED_TRIP) == 2
    P = S.real.astype(np.float64) ** 2 + S.imag.astype(np.float64) ** 2
    assert P.reshape(-1).argmax() == R.SPEC_PEAK[0] * R.SPEC_T + R.SPEC_PEAK[1] > 2 * R.MAX_STRIDED_TRIP
    first = P.reshape(-1)[:R.MAX_STRIDED_TRIP].max()
    flips = int((R.ibm_exact(S, max_power=first)[0] != mask).sum())
    mags = np.sqrt(P[P > 0])
    print("spectrum: %.1f %% ones, %d undecided, the first trip's maximum alone flips %d labels, |S| over %.1f decades"
          % (100 * mask.mean(), undecided.sum(), flips, np.log10(mags.max() / mags.min())))
    assert undecided.sum() == 0 and 0.10 <= mask.mean() <= 0.90 and flips >= 1000
    assert np.log10(mags.max() / np.percentile(mags, 1)) >= 3
    tail = mask.reshape(-1)[R.MASK_STRIDED_TRIP:]
    assert 0.10 <= tail.mean() <= 0.90 and 0.3 <= vad.mean() <= 0.7
    # the restatement is the reference's mask wherever the float64 dB comparison is not within rounding of the threshold
    ref, mag, M, tau = R.ibm_parts(S, np.float64(np.float32(1e-8)), 50)
    assert not ((ref != mask) & (np.abs(mag - tau) > 1e-9 * M)).any()


def test_noise_aware_batch_reaches_what_it_aims_at():
    """the last frames of row 1 (all that noise_aware_mask's second trip writes) hold both values of both masks"""
    import noise_aware_ref as NA
    from avvad import ops
    n = R.NA_B * R.NA_T * 513
    assert R.trips(n, R.MASK_TRIP) == 2
    first = (R.MASK_TRIP - R.NA_T * 513) // 513                       # row 1's first frame with an output of the second trip
    assert 5000 <= first < R.NA_T
    X, N = R.noise_aware_row(1)
    cs, cn = ops.noise_aware_tables(513)
    speech, noise, irm = NA.noise_aware(X[first:], N[first:], cs, cn, peak=np.array([2.5], np.float32))
    print("noise-aware row 1 from frame %d: %.1f %% speech, %.1f %% noise" % (first, 100 * speech.mean(), 100 * noise.mean()))
    assert 0.10 <= speech.mean() <= 0.90 and 0.10 <= noise.mean() <= 0.90 and 0.1 < irm.mean() < 0.9


def test_target_frames_refuses_an_utterance_shorter_than_a_frame():
    from avvad import ops
    from avvad._lib import AvvadError
    with pytest.raises(AvvadError, match="500 samples"):
        ops.target_frames(500)
    with pytest.raises(AvvadError):
        ops.target_frames(600, pad_at_end=False)
    assert ops.target_frames(1024) == (1024, 1) and ops.target_frames(L=1023) == (1279, 1)      # one hop of end pad makes a frame


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
