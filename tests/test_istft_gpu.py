"""The masked inverse STFT on the GPU against the float64 oracle of tests/istft_ref.py.

Outputs are compared through the numerator, ``E = max_s |y_gpu[s] wss64[s] - num64[s]|`` over EVERY sample (the first and
last samples divide by hann^2 down to 8.9e-11, where float32 itself is off by 8e-3), and the bound is ``8 * E_cpu32``:
the same measure of a float32 CPU evaluation of the GEMM form on the same input (``istft_ref.istft32_gemm``).  Observed
``E`` and the bound go to the parity log.  Exact properties -- zeros behind a row's length, mask mode 3 against the 0/1
mask, the fused call against its two halves, run to run -- are compared bit for bit."""
import os

import numpy as np
import pytest
import torch

import istft_ref as R
from conftest import GOLDEN, load_golden

from test_gpu_parity import _report as _parity_report

pytestmark = pytest.mark.gpu
T_ = torch.from_numpy
DEV = "cuda:0"


def _report(name, got, ref, atol):
    _parity_report("istft: " + name, got, ref, atol)


def _check_row(name, y_gpu, S64, n_fft, hop, center=False, length=None, scale=1.0):
    """one output row against the oracle of its (masked) float64 spectrum, bound 8 E_cpu32 of the same spectrum"""
    y_gpu = y_gpu.detach().cpu().numpy() if isinstance(y_gpu, torch.Tensor) else y_gpu
    _, num, wss = R.istft64(S64, n_fft, hop, center=center, length=length)
    e32 = R.weighted_error(R.istft32_gemm(S64, n_fft, hop, center=center, length=length), num, wss)[0]
    e, got, ref = R.weighted_error(y_gpu, num, wss, scale)
    print("istft: %-40s E = %.3e  E_cpu32 = %.3e  ratio %.2f" % (name, e, e32, e / e32))
    assert e32 > 0
    _report(name, got, ref, R.FACTOR * e32 * abs(scale))
    return e, e32


def _batch(n_fft, hop, frames, seed, fill=float("nan")):
    """ragged rows of random spectra: (list of complex64 (T_b, F), GPU (B, Tmax, F, 2) whose padding frames hold `fill`)"""
    rng = np.random.default_rng(seed)
    rows = [R.random_spectrum(rng, T, n_fft) for T in frames]
    spec = np.full((len(frames), max(frames), n_fft // 2 + 1, 2), fill, dtype=np.float32)
    for b, S in enumerate(rows):
        spec[b, :S.shape[0], :, 0], spec[b, :S.shape[0], :, 1] = S.real, S.imag
    return rows, T_(spec).to(DEV)


def _logits(rng, shape):
    """|logit| >= 0.1: no threshold and no rounding of the sigmoid can flip a decision"""
    z = rng.standard_normal(shape)
    return (np.sign(z) * (0.1 + 2.0 * np.abs(z))).astype(np.float32)


PARITY = [(64, 16, [9, 4, 1]), (96, 24, [7, 2]), (64, 48, [5, 3]), (1024, 256, [130, 5])]


@pytest.mark.parametrize("n_fft,hop,frames", PARITY)
def test_parity_with_the_oracle_and_exact_zeros(n_fft, hop, frames):
    """mask_mode 0 on ragged batches: a one-frame row, an FFT length that is no power of two, a hop that does not divide the
    FFT length, and B T = 260 rows across the engine's 128-row tiles.  The padding frames of the shorter rows hold NaN:
    nothing of them may reach the output, which is exactly zero behind each row's own length."""
    from avvad import ops
    rows, spec = _batch(n_fft, hop, frames, seed=n_fft + hop)
    out = ops.istft(spec, n_fft, hop, n_frames=frames)
    Lmax = R.istft_length(max(frames), n_fft, hop)
    assert out.shape == (len(frames), Lmax) and out.dtype == torch.float32
    for b, S in enumerate(rows):
        natural = R.istft_length(frames[b], n_fft, hop)
        assert torch.count_nonzero(out[b, natural:]).item() == 0 and not torch.signbit(out[b, natural:]).any()
        _check_row("parity %d/%d row %d (%d frames)" % (n_fft, hop, b, frames[b]), out[b], S.astype(np.complex128), n_fft, hop,
                   length=Lmax)
    # a row without frames is all zeros
    none = ops.istft(spec, n_fft, hop, n_frames=[0] * len(frames), length=Lmax)
    assert torch.count_nonzero(none).item() == 0


@pytest.mark.parametrize("n_fft,hop,frames", [(64, 16, [9, 4]), (1024, 256, [6])])
def test_mask_modes(n_fft, hop, frames):
    """mode 1 (given mask), 2 (sigmoid of logits) and 3 (logits > 0) against the oracle of the float64-masked spectrum; mode 3
    is bit-equal to mode 1 with the 0/1 mask of the same logits."""
    from avvad import ops
    rows, spec = _batch(n_fft, hop, frames, seed=7 + n_fft, fill=0.0)
    rng = np.random.default_rng(n_fft)
    B, Tm, F = len(frames), max(frames), n_fft // 2 + 1
    mask = rng.random((B, Tm, F)).astype(np.float32)
    logit = _logits(rng, (B, Tm, F))
    soft64 = 1.0 / (1.0 + np.exp(-logit.astype(np.float64)))
    hard = (logit > 0).astype(np.float32)
    assert 0.2 < hard.mean() < 0.8
    L = R.istft_length(Tm, n_fft, hop)
    outs = {1: ops.istft(spec, n_fft, hop, mask=T_(mask).to(DEV), n_frames=frames),
            2: ops.istft(spec, n_fft, hop, mask=T_(logit).to(DEV), mask_mode=2, n_frames=frames),
            3: ops.istft(spec, n_fft, hop, mask=T_(logit).to(DEV), mask_mode=3, n_frames=frames)}
    for mode, m64 in ((1, mask.astype(np.float64)), (2, soft64), (3, hard.astype(np.float64))):
        for b, S in enumerate(rows):
            _check_row("mask mode %d %d/%d row %d" % (mode, n_fft, hop, b), outs[mode][b],
                       S.astype(np.complex128) * m64[b, :frames[b]], n_fft, hop, length=L)
    as_mask = ops.istft(spec, n_fft, hop, mask=T_(hard).to(DEV), mask_mode=1, n_frames=frames)
    assert torch.equal(outs[3], as_mask)
    assert not torch.equal(outs[3], outs[2])


def _covered(y, x, L, natural, hop):
    """(got, ref) weighted by the constant window sum of squares over the fully covered samples [3 hop, L' - 3 hop)"""
    lo, hi = 3 * hop, min(L, natural - 3 * hop)
    assert hi - lo > 4 * hop
    return 1.5 * np.asarray(y[lo:hi], dtype=np.float64), 1.5 * np.asarray(x[lo:hi], dtype=np.float64)


def test_round_trip_returns_the_waveform():
    """ops.resynth(x, mask_mode 0) against x on the samples every frame position covers (hop = n_fft / 4: the window sum of
    squares is 1.5 there), under the same rule with E_cpu32 from the float32 CPU round trip.  L = 5000 takes the end-pad
    branch of the frame count, 5120 does not, 3000 leaves its row short of the batch's pitch; every row comes back with
    exactly its own number of samples."""
    from avvad import ops
    n_fft, hop, lens = 1024, 256, [5000, 5120, 3000]
    rng = np.random.default_rng(11)
    x = np.zeros((3, 5120), dtype=np.float32)
    for b, n in enumerate(lens):
        v = rng.standard_normal(n)
        x[b, :n] = v / np.abs(v).max()
    out = ops.resynth(T_(x).to(DEV), None, mask_mode=0, n_fft=n_fft, hop=hop, sample_lengths=lens)
    assert out.shape == (3, 5120)
    y = out.cpu().numpy()
    bounds = []
    for b, n in enumerate(lens):
        assert not y[b, n:].any()
        natural = R.istft_length(ops.n_frames(n, n_fft, hop), n_fft, hop)
        assert natural >= n
        y32 = R.istft32_gemm(R.stft32_gemm(x[b, :n], n_fft, hop), n_fft, hop)
        g32, ref = _covered(y32, x[b], n, natural, hop)
        e32 = float(np.abs(g32 - ref).max())
        got, ref = _covered(y[b], x[b], n, natural, hop)
        print("istft: round trip L = %d  E = %.3e  E_cpu32 = %.3e" % (n, np.abs(got - ref).max(), e32))
        _report("round trip L = %d" % n, got, ref, R.FACTOR * e32)
        bounds.append(R.FACTOR * e32)
    # default lengths: every row is the whole pitch
    whole = ops.resynth(T_(x[1]).to(DEV), None, mask_mode=0)
    assert whole.shape == (1, 5120)
    got, ref = _covered(whole[0].cpu().numpy(), x[1], 5120, 5120, hop)
    _report("round trip, default lengths", got, ref, bounds[1])


def test_fused_call_equals_its_halves_and_runs_are_reproducible():
    from avvad import ops
    n_fft, hop, lens = 1024, 256, [9000, 7300]
    rng = np.random.default_rng(3)
    w = np.zeros((2, 9000), dtype=np.float32)
    for b, n in enumerate(lens):
        w[b, :n] = rng.standard_normal(n) * 0.2
    w = T_(w).to(DEV)
    T = ops.n_frames(9000, n_fft, hop)
    m = T_(rng.random((2, T, 513)).astype(np.float32)).to(DEV)
    fused = ops.resynth(w, m, sample_lengths=lens)
    spec = ops.stft_complex(w, n_fft, hop)
    assert spec.shape == (2, T, 513, 2)
    one = ops.stft_complex(w[1], n_fft, hop)
    assert torch.equal(one[0].permute(1, 0, 2), ops.stft(w[1], n_fft, hop, mode=2))       # the spectrum of the front-end
    halves = ops.istft(spec, n_fft, hop, mask=m, n_frames=[ops.n_frames(n, n_fft, hop) for n in lens], length=lens)
    assert halves.shape == fused.shape == (2, 9000)
    assert torch.equal(fused, halves)
    assert torch.equal(fused, ops.resynth(w, m, sample_lengths=lens))
    assert torch.equal(halves, ops.istft(spec, n_fft, hop, mask=m, n_frames=[ops.n_frames(n, n_fft, hop) for n in lens], length=lens))


def test_a_row_alone_agrees_with_the_batched_row():
    from avvad import ops
    for n_fft, hop, frames in ((64, 16, [9, 4, 1]), (1024, 256, [130, 5])):
        rows, spec = _batch(n_fft, hop, frames, seed=21, fill=0.0)
        Lmax = R.istft_length(max(frames), n_fft, hop)
        batched = ops.istft(spec, n_fft, hop, n_frames=frames).cpu().numpy()
        for b, S in enumerate(rows):
            alone = ops.istft(spec[b:b + 1, :frames[b]].contiguous(), n_fft, hop, length=Lmax)[0].cpu().numpy()
            _, num, wss = R.istft64(S.astype(np.complex128), n_fft, hop, length=Lmax)
            e32 = R.weighted_error(R.istft32_gemm(S, n_fft, hop, length=Lmax), num, wss)[0]
            w = np.where(wss > R.TINY32, wss, 1.0)
            _report("row %d alone vs batched %d/%d" % (b, n_fft, hop), alone * w, batched[b] * w, R.FACTOR * e32)


def test_length_center_and_scale():
    from avvad import ops
    n_fft, hop, T = 64, 16, 9
    rows, spec = _batch(n_fft, hop, [T, T], seed=5)
    S = [r.astype(np.complex128) for r in rows]
    natural = R.istft_length(T, n_fft, hop)
    assert natural == 192
    for name, kw in (("crop", dict(length=100)), ("zero-fill", dict(length=natural + 37)), ("center", dict(center=True)),
                     ("center + crop", dict(center=True, length=90)), ("center + zero-fill", dict(center=True, length=200))):
        out = ops.istft(spec, n_fft, hop, **kw)
        want = kw.get("length", R.istft_length(T, n_fft, hop, kw.get("center", False)))
        assert out.shape == (2, want), name
        filled = natural - (n_fft // 2 if kw.get("center") else 0)
        assert torch.count_nonzero(out[:, filled:]).item() == 0, name
        for b in range(2):
            _check_row("%s row %d" % (name, b), out[b], S[b], n_fft, hop, center=kw.get("center", False), length=want)
    plain = ops.istft(spec, n_fft, hop)
    assert torch.equal(ops.istft(spec, n_fft, hop, center=True), plain[:, n_fft // 2:natural - n_fft // 2])
    assert torch.equal(ops.istft(spec, n_fft, hop, length=[100, 150])[0, :100], plain[0, :100])
    ragged = ops.istft(spec, n_fft, hop, length=[100, 150])
    assert ragged.shape == (2, 150) and torch.count_nonzero(ragged[0, 100:]).item() == 0 and torch.equal(ragged[1], plain[1, :150])
    scale = torch.tensor([2.5, 0.3], device=DEV)
    scaled = ops.istft(spec, n_fft, hop, scale=scale)
    assert torch.equal(scaled, plain * scale[:, None])                       # one float32 multiplication, nothing else
    _check_row("scale 0.3", scaled[1], S[1], n_fft, hop, scale=float(np.float32(0.3)))


def test_legacy_layouts_round_trip():
    """packages.processing.stft.istft on what stft_pytorch returns -- the (F, T, 2) view and its complex twin -- with
    center=False on both sides; then the reference's defaults (center=True on both sides), max_len as a sample count."""
    from avvad import ops
    from packages.processing.stft import istft, stft_pytorch
    n_fft, hop, L = 1024, 256, 5000
    rng = np.random.default_rng(17)
    v = rng.standard_normal(L)
    x = (v / np.abs(v).max()).astype(np.float32)
    xg = T_(x).to(DEV)
    kw = dict(fs=16000, wlen_sec=64e-3, hop_percent=0.25)
    S = stft_pytorch(xg, center=False, **kw)
    T = ops.n_frames(L, n_fft, hop)
    assert S.shape == (513, T, 2)
    y = istft(S, center=False, **kw)
    natural = R.istft_length(T, n_fft, hop)
    assert y.shape == (natural,) and y.dtype == torch.float32
    assert torch.equal(y, istft(torch.view_as_complex(S), center=False, **kw))
    assert torch.equal(y, ops.istft(S.permute(1, 0, 2).contiguous()[None], n_fft, hop)[0])       # the batched layout
    y32 = R.istft32_gemm(R.stft32_gemm(x, n_fft, hop), n_fft, hop)
    g32, ref = _covered(y32, x, L, natural, hop)
    got, ref = _covered(y.cpu().numpy(), x, L, natural, hop)
    _report("legacy (F,T,2) round trip", got, ref, R.FACTOR * float(np.abs(g32 - ref).max()))
    # max_len is librosa's `length`: samples.  The reference's x[:int(max_len * fs)] behind it cuts nothing.
    assert istft(S, center=False, max_len=4000, **kw).shape == (4000,)
    assert torch.equal(istft(S, center=False, max_len=4000, **kw), y[:4000])
    Sc = stft_pytorch(xg, center=True, **kw)
    yc = istft(Sc, max_len=L, **kw)
    assert yc.shape == (L,)
    wss_c = 1.5                                                                # centred frames cover every sample of x fully
    lo, hi = hop, L - hop
    x_pad = np.pad(np.concatenate([x, np.zeros(hop, np.float32)]), n_fft // 2, mode="reflect")
    y32c = R.istft32_gemm(R.stft32_gemm(x_pad, n_fft, hop, pad_at_end=False), n_fft, hop, center=True, length=L)
    e32 = float(np.abs(wss_c * (y32c[lo:hi].astype(np.float64) - x[lo:hi])).max())
    _report("centred round trip", wss_c * yc.cpu().numpy()[lo:hi].astype(np.float64), wss_c * x[lo:hi].astype(np.float64), R.FACTOR * e32)


def test_evaluator_writes_the_enhanced_utterance(tmp_path):
    from scipy.io import wavfile
    from avvad import train as TR
    from packages.models.Audio_Net import DeepVAD_audio
    g = load_golden("eval_audio")
    wav = os.path.join(GOLDEN, "utt_sa1.npz")
    ck = os.path.join(GOLDEN, "audio_ref_h32_y513.pt")
    stats = TR.Stats(audio_mean=g["mean"], audio_std=g["std"])
    make = lambda: DeepVAD_audio(2, 32, 513)      # noqa: E731
    TR.evaluate_main("audio", make, checkpoint=ck, out_dir=str(tmp_path / "a"), wav_list=[wav], stats=stats)
    TR.evaluate_main("audio", make, checkpoint=ck, out_dir=str(tmp_path / "b"), wav_list=[wav], stats=stats,
                     resynth_dir=str(tmp_path / "wav"))
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == ["utt_sa1_y_hat_hard.pt", "utt_sa1_y_hat_soft.pt"]
    for f in os.listdir(tmp_path / "a"):
        assert torch.equal(torch.load(tmp_path / "a" / f, weights_only=True), torch.load(tmp_path / "b" / f, weights_only=True))
    assert os.listdir(tmp_path / "wav") == ["utt_sa1_enhanced.wav"]
    fs, y = wavfile.read(str(tmp_path / "wav" / "utt_sa1_enhanced.wav"))
    x_t, _ = TR.load_waveform(wav)
    assert fs == 16000 and y.dtype == np.float32 and y.shape == (x_t.numel(),) == (48100,)
    assert np.isfinite(y).all()
    print("istft: enhanced utt_sa1 peak %.3f (input %.3f)" % (np.abs(y).max(), float(x_t.abs().max())))
    model = make()
    model.load_state_dict(torch.load(ck, map_location="cpu", weights_only=True))
    model = model.to(DEV).eval()
    with torch.no_grad():
        direct = TR.resynth_utt(model, x_t.to(DEV), stats, hard=True)
        soft = TR.resynth_utt(model, x_t.to(DEV), stats, hard=False)
    assert np.array_equal(direct.cpu().numpy(), y)
    assert soft.shape == direct.shape and torch.isfinite(soft).all() and not torch.equal(soft, direct)
    TR.evaluate_main("audio", make, checkpoint=ck, out_dir=str(tmp_path / "c"), wav_list=[wav], stats=stats,
                     resynth_dir=str(tmp_path / "wav_soft"), resynth_hard=False)
    assert np.array_equal(wavfile.read(str(tmp_path / "wav_soft" / "utt_sa1_enhanced.wav"))[1], soft.cpu().numpy())
