"""GPU tests of the noise-aware masks (csrc/target.hip noise_aware_mask, ops.noise_aware_targets /
noise_aware_from_spectrum, the drop-ins noise_aware_IBM / threshold_IBM, ``mix_labels`` of the training step).

From given float32 spectra every step of the kernel is exactly rounded double arithmetic, as in tests/noise_aware_ref.py,
so those results are compared bit for bit.  From waveforms the spectra are the DFT GEMM's, and the masks are compared
with the float64 restatement and with the reference's own results (tests/golden/noise_aware.npz) outside the rounding
band that tests/test_noise_aware_cpu.py defines."""
import os
import re

import numpy as np
import pytest
import torch

import noise_aware_ref as R
from conftest import GOLDEN
from test_mix_gpu import _files
from test_noise_aware_cpu import BAND_CAP, banded_mismatches, sa1_case, sa1_pair
from test_targets_cpu import IBM_DELTA

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = 513
NAMES = ("speech", "noise", "irm")


def _ops():
    from avvad import ops
    return ops


def _tables():
    return _ops().noise_aware_tables(F)


def _np_complex(t):
    """(.., 2) float32 or complex64 tensor -> complex64 numpy"""
    t = t if t.is_complex() else torch.view_as_complex(t.contiguous())
    return t.cpu().numpy()


def _check_exact(got, X, N, what, **kw):
    """all three outputs against the restatement on the same float32 spectra, bit for bit"""
    cs, cn = _tables()
    speech, noise, irm = R.noise_aware(X, N, cs, cn, **kw)
    want = dict(speech=speech.astype(np.float32), noise=noise.astype(np.float32), irm=irm)
    for k in got:
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape and g.dtype == np.float32, (what, k)
        bad = g.view(np.int32) != want[k].view(np.int32)
        assert not bad.any(), "%s %s: %d of %d values differ" % (what, k, bad.sum(), bad.size)


def _spectra():
    """X, N complex64 (2, 3, 513): magnitudes over four decades (thresholds, floor and cuts all decide somewhere), a cell
    with X == N on a bin whose speech threshold is 1, and all-zero cells"""
    rng = np.random.default_rng(17)

    def one():
        z = (rng.standard_normal((2, 3, F)) + 1j * rng.standard_normal((2, 3, F))) * 10.0 ** rng.uniform(-3, 1, (2, 3, F))
        return z.astype(np.complex64)
    X, N = one(), one()
    assert _tables()[0][100] == 1.0
    N[0, 1, 100] = X[0, 1, 100]
    X[1, 2, 50] = N[1, 2, 50] = 0
    X[0, 0, 300] = N[0, 0, 300] = 0
    return X, N


def test_exact_from_spectra():
    ops = _ops()
    X, N = _spectra()
    Xd, Nd = torch.from_numpy(X).to(DEV), torch.from_numpy(N).to(DEV)
    peak = torch.tensor([0.37, 2.5], device=DEV)
    # contiguous complex tensors, without and with a peak, with frame counts, and the constant noise power
    _check_exact(ops.noise_aware_from_spectrum(Xd, Nd, outputs=NAMES), X, N, "contiguous")
    got = ops.noise_aware_from_spectrum(Xd, Nd, outputs=NAMES, peak=peak)
    _check_exact(got, X, N, "peak", peak=peak.cpu().numpy())
    assert got["speech"][0, 1, 100] == 0 and got["irm"][0, 1, 100] == 0.5            # X == N, c == 1: strict >
    for b, t, f in ((1, 2, 50), (0, 0, 300)):                                           # all-zero cells
        assert got["speech"][b, t, f] == 0 and got["noise"][b, t, f] == 1 and got["irm"][b, t, f] == 0
    _check_exact(ops.noise_aware_from_spectrum(Xd, Nd, outputs=NAMES, n_frames=[3, 1], peak=peak), X, N, "ragged",
                 peak=peak.cpu().numpy(), n_frames=[3, 1])
    _check_exact(ops.noise_aware_from_spectrum(Xd, None, outputs=NAMES, peak=peak), X, None, "threshold", peak=peak.cpu().numpy())
    assert 0 < int(ops.noise_aware_from_spectrum(Xd, None, outputs=("speech",))["speech"].sum()) < X.size // 2
    for bad_peak in (0.0, float("inf"), float("nan")):                                  # no scaling
        pk = torch.tensor([bad_peak, 1.0], device=DEV)
        _check_exact(ops.noise_aware_from_spectrum(Xd, Nd, outputs=NAMES, peak=pk), X, N, "peak %r" % bad_peak)
    # other cuts, floor and thresholds
    cs, cn = ops.noise_aware_tables(F, 7, 1, -12, -8)
    sp, nz, _ = R.noise_aware(X, N, cs, cn, low_cut=1, high_cut=513, floor=0.5)
    got = ops.noise_aware_from_spectrum(Xd, Nd, outputs=("noise", "speech"), threshold_unvoiced_speech=7, threshold_voiced_speech=1,
                                        threshold_unvoiced_noise=-12, threshold_voiced_noise=-8, low_cut=1, high_cut=513, floor=0.5)
    assert list(got) == ["noise", "speech"]
    assert np.array_equal(got["speech"].cpu().numpy() != 0, sp) and np.array_equal(got["noise"].cpu().numpy() != 0, nz)
    # the legacy (F, T, 2) view of one utterance, transposed in through its strides
    legacy_x = torch.view_as_real(Xd[1]).permute(1, 0, 2).contiguous()                   # (F, T, 2)
    legacy_n = torch.view_as_real(Nd[1]).permute(1, 0, 2).contiguous()
    vx, vn = legacy_x.permute(1, 0, 2), legacy_n.permute(1, 0, 2)
    assert vx.stride() == (2, 6, 1)
    got = ops.noise_aware_from_spectrum(vx, vn, outputs=NAMES)
    assert got["irm"].shape == (3, F)
    _check_exact(got, X[1], N[1], "legacy view")
    # a column slice of a wider tensor (and an unsliced noise)
    wide = torch.full((2, 3, F + 7), float("nan"), dtype=torch.complex64, device=DEV)
    wide[:, :, 3:3 + F] = Xd
    _check_exact(ops.noise_aware_from_spectrum(wide[:, :, 3:3 + F], Nd, outputs=NAMES, peak=peak), X, N, "column slice",
                 peak=peak.cpu().numpy())
    # one output at a time gives the same values
    for k in NAMES:
        _check_exact(ops.noise_aware_from_spectrum(Xd, Nd, outputs=(k,)), X, N, "only " + k)


def test_exact_past_one_grid_stride_trip():
    """noise_aware_mask on B * T * F = 2 * 8201 * 513 = 8,414,226 outputs: two trips of the grid-stride loop (8192
    workgroups x 256 threads x 4 outputs a trip).  With n_frames = [8201, 5000] the second trip (row 1 from frame 8151 on)
    writes zeros behind the row's frames; with [5000, 8201] it decides live cells.  Both bit for bit, all three outputs,
    with a peak per row; the reference one row at a time."""
    import target_ref as TR
    ops = _ops()
    assert TR.trips(TR.NA_B * TR.NA_T * F, TR.MASK_TRIP) == 2
    rows = [TR.noise_aware_row(b) for b in range(TR.NA_B)]
    Xd = torch.from_numpy(np.stack([r[0] for r in rows])).to(DEV)
    Nd = torch.from_numpy(np.stack([r[1] for r in rows])).to(DEV)
    peak = torch.tensor([0.37, 2.5], device=DEV)
    pk = peak.cpu().numpy()
    for counts in ([8201, 5000], [5000, 8201]):
        got = ops.noise_aware_from_spectrum(Xd, Nd, n_frames=counts, peak=peak, outputs=NAMES)
        for b in range(TR.NA_B):
            _check_exact({k: v[b:b + 1] for k, v in got.items()}, rows[b][0][None], rows[b][1][None], "n_frames %r row %d" % (counts, b),
                         peak=pk[b:b + 1], n_frames=counts[b:b + 1])
            assert all(not got[k][b, counts[b]:].any() for k in NAMES), (counts, b)
        print("noise-aware %r: %d outputs a mask, 0 excluded (bit for bit)" % (counts, got["speech"].numel()))
        del got


def test_a_row_shorter_than_a_frame_is_refused():
    """ops.target_frames raises AvvadError for such a row, so noise_aware_targets returns before any launch"""
    from avvad._lib import AvvadError
    ops = _ops()
    wave = torch.zeros(2, 5000, device=DEV)
    with pytest.raises(AvvadError, match="shorter than one"):
        ops.noise_aware_targets(wave, wave, [5000, 500])


def _ragged():
    """four rows, width 4000: one frame, an end pad, the longest, and an all-zero row"""
    rng = np.random.default_rng(23)
    lens = [1024, 1500, 4000, 2000]
    speech = np.zeros((4, 4000), np.float32)
    noise = np.zeros((4, 4000), np.float32)
    t = np.arange(4000)
    for b, n in enumerate(lens):
        speech[b, :n] = (np.sin(2 * np.pi * (200 + 150 * b) * t[:n] / 16000) * (0.2 + 0.8 * rng.random()) +
                         0.05 * rng.standard_normal(n)) * np.hanning(n)
        noise[b, :n] = 0.1 * rng.standard_normal(n)
    speech[3] = 0
    return lens, speech, noise


def test_waveform_path_is_the_spectrum_path():
    ops = _ops()
    lens, speech, noise = _ragged()
    s, n = torch.from_numpy(speech).to(DEV), torch.from_numpy(noise).to(DEV)
    peak = torch.from_numpy(np.abs(speech + noise).max(axis=1)).to(DEV)
    frames, got = ops.noise_aware_targets(s, n, lens, peak=peak, outputs=NAMES)
    assert frames.tolist() == [1, 3, 13, 5] == [ops.target_frames(v)[1] for v in lens]
    X, N = ops.stft_complex(s), ops.stft_complex(n)
    assert X.shape == (4, 13, F, 2)
    want = ops.noise_aware_from_spectrum(X, N, n_frames=frames.tolist(), peak=peak, outputs=NAMES)
    for k in NAMES:
        assert got[k].shape == (4, 13, F) and torch.equal(got[k], want[k]), k
        for b, T in enumerate(frames.tolist()):
            assert not got[k][b, T:].any(), (k, b)
    _check_exact(got, _np_complex(X), _np_complex(N), "waveform", peak=peak.cpu().numpy(), n_frames=frames.tolist())
    # the silent row inside its frames
    assert not got["speech"][3, :5].any() and got["noise"][3, :5].all() and not got["irm"][3, :5].any()
    # without a peak, and a single row as a 1-D wave
    _, plain = ops.noise_aware_targets(s, n, lens, outputs=("irm",))
    assert torch.equal(plain["irm"], ops.noise_aware_from_spectrum(X, N, n_frames=frames.tolist(), outputs=("irm",))["irm"])
    f1, one = ops.noise_aware_targets(s[2], n[2], [4000])
    assert list(one) == ["speech"] and one["speech"].shape == (1, 13, F) and f1.tolist() == [13]


def test_sa1_pair_against_the_reference_and_the_drop_ins():
    from packages.processing.target import noise_aware_IBM, threshold_IBM
    ops = _ops()
    c = sa1_case()
    s, n = (torch.from_numpy(x).to(DEV) for x in sa1_pair())
    frames, got = ops.noise_aware_targets(s, n, [s.numel()], outputs=("speech", "noise"))
    assert frames.tolist() == [185]
    X = torch.view_as_complex(ops.stft_complex(s))[0]
    N = torch.view_as_complex(ops.stft_complex(n))[0]
    # the GEMM's spectra lie within the DFT bound the band is built on
    for Z, Z64 in ((X, c["X"]), (N, c["N"])):
        err = np.abs(Z.cpu().numpy().astype(np.complex128) - Z64).max()
        print("max |S - S64| = %.2e of max|S| (bound %.0e)" % (err / np.abs(Z64).max(), IBM_DELTA))
        assert err <= IBM_DELTA * np.abs(Z64).max()
    thr = threshold_IBM(X)
    assert thr.dtype == torch.bool and thr.is_cuda and thr.shape == (185, F)
    ours = dict(speech=got["speech"][0].cpu().numpy() != 0, noise=got["noise"][0].cpu().numpy() != 0, threshold=thr.cpu().numpy())
    for k, mask in ours.items():
        band = c["band"][k]
        frac = band[:, c["inside"]].mean()
        print("%s: %.3f %% of the cells between the cuts in the band, %d cells differ in all"
              % (k, 100 * frac, (mask != c["masks"][k]).sum()))
        assert frac <= BAND_CAP
        assert banded_mismatches(mask, c["masks"][k], band) == 0, k
        assert np.array_equal(mask[:, ~c["inside"]], c["masks"][k][:, ~c["inside"]])
    # drop-ins: GPU in / GPU out and numpy in / numpy out agree, and equal the batched labels
    sp_t, nz_t = noise_aware_IBM(X, N)
    assert sp_t.dtype == nz_t.dtype == torch.bool and sp_t.is_cuda
    sp_n, nz_n = noise_aware_IBM(X.cpu().numpy(), N.cpu().numpy())
    assert isinstance(sp_n, np.ndarray) and sp_n.dtype == nz_n.dtype == np.bool_
    assert np.array_equal(sp_n, sp_t.cpu().numpy()) and np.array_equal(nz_n, nz_t.cpu().numpy())
    assert np.array_equal(sp_n, ours["speech"]) and np.array_equal(nz_n, ours["noise"])
    thr_n = threshold_IBM(X.cpu().numpy())
    assert isinstance(thr_n, np.ndarray) and thr_n.dtype == np.bool_ and np.array_equal(thr_n, ours["threshold"])


def test_row_alone_and_run_to_run():
    ops = _ops()
    lens, speech, noise = _ragged()
    s, n = torch.from_numpy(speech).to(DEV), torch.from_numpy(noise).to(DEV)
    frames, batch = ops.noise_aware_targets(s, n, lens, outputs=NAMES)
    _, again = ops.noise_aware_targets(s, n, lens, outputs=NAMES)
    for k in NAMES:
        assert torch.equal(batch[k], again[k]), k
    cs, cn = _tables()
    for b, L in enumerate(lens):
        f1, single = ops.noise_aware_targets(s[b:b + 1, :L].contiguous(), n[b:b + 1, :L].contiguous(), [L], outputs=NAMES)
        T = int(f1[0])
        assert T == int(frames[b])
        # the DFT GEMM's stream-K split depends on the batch's row count: a cell may fall to the other side only in the band
        bands = R.bands(R.dft64(speech[b, :L]), R.dft64(noise[b, :L]), cs, cn, IBM_DELTA)
        for k, band in zip(("speech", "noise"), bands):
            diff = (batch[k][b, :T] != single[k][0]).cpu().numpy()
            assert not (diff & ~band).any(), (k, b)


def _three_clean(tmp_path):
    clean, _ = _files(tmp_path)
    return clean + [os.path.join(GOLDEN, "utt_sa1_clean.npz")]


def test_mix_step_labels(tmp_path):
    from avvad import train as TR
    ops = _ops()
    dev = torch.device(DEV)
    paths = _three_clean(tmp_path)
    bank = TR.read_noise_bank(str(tmp_path / "noise.txt"), dev)
    ds = TR.CleanWavs(paths)
    batch = TR.CleanWavs.collate([ds[0], ds[1], ds[2]])
    lens = [int(v) for v in batch[0]]
    mixer = TR.MixDraw(bank, (-5.0, 20.0), mix_seed=3, rank=0)
    clip, start, snr = mixer.seed(2)(lens)
    clean = ops.peak_normalize(batch[1].to(dev))
    noisy, noise, info = ops.mix(clean, lens, bank, clip, start, snr, return_noise=True, return_info=True)
    base = TR.mix_step(batch, dev, "ibm_labels", bank, mixer.seed(2))
    same = TR.mix_step(batch, dev, "ibm_labels", bank, mixer.seed(2), mix_labels="clean")
    want_frames, want_clean = ops.speech_targets(clean, lens, "ibm_labels", center=False, pad_at_end=True, eps=1e-8)
    assert torch.equal(base[2], want_clean) and torch.equal(base[0].cpu(), want_frames)
    assert all(torch.equal(a, b) for a, b in zip(base, same))
    for name, key in (("noise_aware", "speech"), ("irm", "irm")):
        frames, x, target, waves = TR.mix_step(batch, dev, "ibm_labels", bank, mixer.seed(2), waves=True, mix_labels=name)
        wf, want = ops.noise_aware_targets(clean, noise, lens, peak=info["peak"], outputs=(key,))
        assert torch.equal(target, want[key]) and torch.equal(frames.cpu(), wf) and torch.equal(x, base[1])
        assert torch.equal(waves[0], ops.peak_normalize(noisy)) and torch.equal(waves[1], clean) and torch.equal(waves[3], noise)
        assert not torch.equal(target, want_clean)
        three = TR.mix_step(batch, dev, "ibm_labels", bank, mixer.seed(2), mix_labels=name)
        assert len(three) == 3 and torch.equal(three[2], target)


@pytest.mark.parametrize("objective", ["bce", "si_sdr"])
def test_training_against_the_ratio_mask(tmp_path, objective):
    """DeepVAD_audio (one LSTM layer, hidden 32, 513 outputs) on two clean crops and two noise clips, 2 epochs with the IRM
    as the label: finite losses, and with the BCE the training loss falls from the first epoch to the second."""
    from avvad import train as TR
    from packages.models.Audio_Net import DeepVAD_audio
    _files(tmp_path)
    out = str(tmp_path / "run")
    TR.train_main("audio", lambda: DeepVAD_audio(1, 32, 513), "irm", epochs=2, batch_size=1, lr=1e-3, out_dir=out,
                  clean_wavs=str(tmp_path / "clean.txt"), noise_wavs=str(tmp_path / "noise.txt"), snr_db=(-5.0, 20.0), mix_seed=4,
                  objective=objective, compute_stats=True, mix_labels="irm")
    log = open(os.path.join(out, "output_batch.log")).read()
    train = [float(v) for v in re.findall(r"train loss (\S+)", log)]
    valid = [float(v) for v in re.findall(r"valid loss (\S+)", log)]
    print(log)
    assert len(train) == len(valid) == 2 and all(np.isfinite(train + valid)), log
    assert ("si-sdr" in log) == (objective == "si_sdr")
    if objective == "bce":
        assert train[1] < train[0], log


def test_masked_bce_takes_a_ratio_mask():
    """avvad_bce_masked against real-valued targets: the formula of csrc/misc.hip in float64,
    sum_b -(1 / (len_b Y)) sum_{t < len_b, y} [x log(sig(r) + eps) + (1 - x) log(1 - sig(r) + eps)], at the tolerances of the
    existing parity tests (1e-4 on the loss, 1e-6 on d/dlogits)."""
    ops = _ops()
    lens, speech, noise = _ragged()
    s, n = torch.from_numpy(speech).to(DEV), torch.from_numpy(noise).to(DEV)
    frames, out = ops.noise_aware_targets(s, n, lens, outputs=("irm",))
    x = out["irm"]
    assert float(x.min()) >= 0 and float(x.max()) <= 1 and int(((x > 0.05) & (x < 0.95)).sum()) > 1000    # real-valued
    gen = torch.Generator().manual_seed(9)
    r = (torch.randn(x.shape, generator=gen) * 2).to(DEV).requires_grad_(True)
    eps = 1e-8
    loss = ops.masked_bce(r, x, frames, eps)
    loss.backward()
    r64 = r.detach().double().cpu().requires_grad_(True)
    x64 = x.double().cpu()
    ref = torch.zeros((), dtype=torch.float64)
    for b, T in enumerate(frames.tolist()):
        sig = torch.sigmoid(r64[b, :T])
        ref = ref - (x64[b, :T] * torch.log(sig + eps) + (1 - x64[b, :T]) * torch.log(1 - sig + eps)).sum() / (T * F)
    ref.backward()
    print("masked BCE against an IRM: %.6f, float64 %.6f" % (float(loss.detach()), float(ref.detach())))
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-4
    assert float((r.grad.double().cpu() - r64.grad).abs().max()) <= 1e-6


def test_ratio_mask_improves_si_sdr():
    """The IRM applied to the normalised 0 dB mixture scores a higher SI-SDR than the mixture: a mask that is inverted,
    transposed or shifted in frequency does not."""
    ops = _ops()
    n_fft, hop, L = 1024, 256, 16000
    c = np.load(os.path.join(GOLDEN, "utt_sa1_clean.npz"))["samples"].astype(np.float32)[14000:14000 + L] / 32768.0
    clean = ops.peak_normalize(torch.from_numpy(c).to(DEV).view(1, -1))
    rng = np.random.default_rng(31)
    bank = ops.NoiseBank([torch.from_numpy(rng.standard_normal(20000).astype(np.float32))], DEV)
    noisy, noise, info = ops.mix(clean, [L], bank, [0], [123], 0.0, return_noise=True, return_info=True)
    mixture = ops.peak_normalize(noisy)
    _, out = ops.noise_aware_targets(clean, noise, [L], peak=info["peak"], outputs=("irm", "noise"))
    skip = n_fft - hop

    def si_sdr(est):
        return float(ops.energy_ratios(est[:, skip:L - skip], clean[:, skip:L - skip])[0, 0])
    base = si_sdr(mixture)
    masked = si_sdr(ops.resynth(mixture, out["irm"], mask_mode=1, n_fft=n_fft, hop=hop, sample_lengths=[L]))
    inverted = si_sdr(ops.resynth(mixture, 1 - out["irm"], mask_mode=1, n_fft=n_fft, hop=hop, sample_lengths=[L]))
    flipped = si_sdr(ops.resynth(mixture, out["irm"].flip(2).contiguous(), mask_mode=1, n_fft=n_fft, hop=hop, sample_lengths=[L]))
    print("SI-SDR dB: mixture %.2f, IRM %.2f, 1 - IRM %.2f, IRM flipped in frequency %.2f" % (base, masked, inverted, flipped))
    assert masked > base
    assert inverted < base and flipped < base
