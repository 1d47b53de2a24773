"""GPU tests of the training labels (csrc/target.hip through avvad.ops and the drop-in packages/processing/target.py):
against the reference's results (tests/golden/targets.npz) outside the stated rounding bands, against the float64
restatement (tests/target_ref.py), ragged batches against single calls, degenerate inputs, reproducibility, and the
real-audio data path of the train / evaluate loops."""
import os

import numpy as np
import pytest
import torch

import target_ref as R
from conftest import GOLDEN, load_golden
from test_targets_cpu import CFGS, IBM_DELTA, ibm_band, sa1, vad_band

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIE = 1e-12          # the GPU sums the squares in float64: it may differ from target_ref only at exact ties


def spectrum64(x):
    """float64 DFT of the end-padded signal (64 ms, center=False): |S|, max|S| for the IBM band."""
    from oracle import frontend
    S = frontend.stft_naive(np.pad(x, (0, 256)) if len(x) % 256 else x, 1024, 256)
    return S


@pytest.mark.parametrize("tag", ["clean", "noisy"])
@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_vad_matches_reference_and_restatement(tag, cfg):
    from packages.processing.target import clean_speech_VAD
    g = load_golden("targets")
    x = sa1(tag)
    gpu = clean_speech_VAD(torch.from_numpy(x).to(DEV), **CFGS[cfg])
    assert gpu.is_cuda and gpu.shape == g["vad_%s_%s" % (tag, cfg)].shape and gpu.dtype == torch.float32
    host = clean_speech_VAD(x, **CFGS[cfg])                 # numpy in -> numpy out, computed on the GPU
    assert isinstance(host, np.ndarray) and host.dtype == np.float32
    v = gpu.cpu().numpy()[0].astype(bool)
    assert np.array_equal(v, host[0].astype(bool))
    E, c = R.vad_energy(x, **CFGS[cfg])
    band = vad_band(E, c)
    assert np.array_equal(v[~band], g["vad_%s_%s" % (tag, cfg)][0].astype(bool)[~band])
    tie = np.abs(E - c * E.min()) <= TIE * c * E.min()
    assert np.array_equal(v[~tie], (E > c * E.min())[~tie])


def test_ibm_both_layouts_match_reference():
    from packages.processing.stft import stft_pytorch
    from packages.processing.target import clean_speech_IBM
    g = load_golden("targets")
    x = sa1("clean")
    legacy = stft_pytorch(torch.from_numpy(x).to(DEV), wlen_sec=64e-3, center=False)          # (F, T, 2) on the GPU
    cplx = torch.view_as_complex(legacy.contiguous())
    S64 = spectrum64(x)
    for thr in (50, 65):
        a = clean_speech_IBM(legacy, ibm_threshold=thr)
        b = clean_speech_IBM(cplx, ibm_threshold=thr)
        assert a.is_cuda and a.shape == (513, 185)
        assert torch.equal(a, b)
        _, mag, M, tau = R.ibm_parts(S64, 1e-8, thr)
        band = ibm_band(mag, M, tau)
        m = a.cpu().numpy().astype(bool)
        print("IBM thr %d: %d of %d bins excluded (delta %.0e)" % (thr, band.sum(), m.size, IBM_DELTA))
        assert band.sum() <= 0.002 * m.size
        assert np.array_equal(m[~band], g["ibm%d_clean" % thr].astype(bool)[~band])
    # the reference's scripts pass a complex numpy array: numpy float32 out
    host = clean_speech_IBM(cplx.cpu().numpy())
    assert isinstance(host, np.ndarray) and np.array_equal(host, clean_speech_IBM(cplx).cpu().numpy())


def test_robust_ibm_is_ibm_times_vad():
    from avvad import ops
    from packages.processing.stft import stft_pytorch
    from packages.processing.target import clean_speech_IBM, clean_speech_VAD, noise_robust_clean_speech_IBM
    x = torch.from_numpy(sa1("clean")).to(DEV)
    kw = dict(wlen_sec=64e-3, center=False)
    S = stft_pytorch(x, **kw)
    ibm, vad = clean_speech_IBM(S), clean_speech_VAD(x, **kw)
    robust = noise_robust_clean_speech_IBM(x, S, **kw)
    assert torch.equal(robust, ibm * vad)
    lens, batched = ops.speech_targets(x.view(1, -1), [x.numel()], "ibm_labels", robust=True)
    assert lens.tolist() == [185] and batched.shape == (1, 185, 513)
    _, plain = ops.speech_targets(x.view(1, -1), [x.numel()], "ibm_labels")
    assert torch.equal(batched[0], plain[0] * vad.view(-1, 1))
    assert torch.equal(plain[0].T, ibm)                  # the waveform path and the spectrum path agree
    with pytest.raises(ValueError):
        noise_robust_clean_speech_IBM(x[:20000], S, **kw)
    from avvad._lib import AvvadError
    with pytest.raises(AvvadError):
        clean_speech_VAD(x, pad_mode="edge")


def five_utterances():
    g = torch.Generator().manual_seed(11)
    loud = torch.randn(9000, generator=g) * 0.3 * 1000.0
    silent_start = torch.cat([torch.zeros(3000), torch.randn(6000, generator=g) * 0.2])
    whole = torch.randn(7680, generator=g) * torch.linspace(0.01, 1.0, 7680)        # 30 hops: no end pad
    zeros = torch.zeros(5000)
    one = torch.randn(1024, generator=g) * 0.5                                      # one 64 ms frame
    return [loud, silent_start, whole, zeros, one]


@pytest.mark.parametrize("labels,robust", [("vad_labels", False), ("ibm_labels", False), ("ibm_labels", True)])
def test_ragged_batch_equals_single_calls(labels, robust):
    from avvad import ops
    utts = five_utterances()
    lens = [u.numel() for u in utts]
    wave = torch.zeros(len(utts), max(lens))
    for i, u in enumerate(utts):
        wave[i, :lens[i]] = u
    frames, batch = ops.speech_targets(wave.to(DEV), lens, labels, robust=robust)
    assert frames.tolist() == [ops.target_frames(n)[1] for n in lens] and frames.tolist()[2] == 27 and frames.tolist()[4] == 1
    for i, u in enumerate(utts):
        f1, single = ops.speech_targets(u.to(DEV).view(1, -1), [lens[i]], labels, robust=robust)
        T = int(f1[0])
        if labels == "vad_labels":
            assert torch.equal(batch[i, :T], single[0]), i
        else:
            # the DFT GEMM's stream-K split depends on the batch's row count: a bin may round to the other side of the
            # threshold only within the IBM band
            diff = (batch[i, :T] != single[0]).cpu().numpy()
            if diff.any():
                x = u.numpy()
                _, mag, M, tau = R.ibm_parts(spectrum64(x), 1e-8, 50)
                assert not (diff & ~ibm_band(mag.T, M, tau)).any(), i
        assert not batch[i, T:].any(), i                   # zeros past T_i
    if labels == "vad_labels":
        assert not batch[3].any()                          # all-zero utterance: VAD all 0
        E, c = R.vad_energy(utts[1].numpy(), wlen_sec=64e-3, center=False)
        assert E.min() == 0.0 and np.array_equal(batch[1, :len(E), 0].cpu().numpy().astype(bool), E > 0)
        # a min leaking across utterances would turn the loud one's threshold into another's
        E0, _ = R.vad_energy(utts[0].numpy(), wlen_sec=64e-3, center=False)
        assert np.array_equal(batch[0, :len(E0), 0].cpu().numpy().astype(bool), E0 > c * E0.min())
    elif not robust:
        assert batch[3, :frames[3]].all()                  # all-zero spectrum: IBM all 1


def test_degenerate_and_edge_fixtures():
    from packages.processing.target import clean_speech_IBM, clean_speech_VAD
    g = load_golden("targets")
    for name in ("silence", "zeros", "whole", "one"):
        v = clean_speech_VAD(torch.from_numpy(g["edge_%s" % name]).to(DEV), wlen_sec=64e-3, center=False)
        assert np.array_equal(v.cpu().numpy().astype(np.uint8), g["edge_vad_%s" % name]), name
    z = torch.zeros(513, 9, dtype=torch.complex64, device=DEV)
    assert torch.equal(clean_speech_IBM(z).cpu(), torch.from_numpy(g["edge_ibm_zeros"]).float())


def test_bit_identical_run_to_run():
    from avvad import ops
    utts = five_utterances()
    lens = [u.numel() for u in utts]
    wave = torch.zeros(len(utts), max(lens))
    for i, u in enumerate(utts):
        wave[i, :lens[i]] = u
    wave = wave.to(DEV)
    for labels in ("vad_labels", "ibm_labels"):
        a = ops.speech_targets(wave, lens, labels, robust=True)[1]
        b = ops.speech_targets(wave, lens, labels, robust=True)[1]
        assert torch.equal(a, b)


# ------------------------------------------------------------------ the real-audio data path
def pair_files(tmp_path):
    """(noisy sa1, clean sa1) and a second, shorter crop of both, as .npz utterances."""
    n = np.load(os.path.join(GOLDEN, "utt_sa1.npz"))["samples"]
    c = np.load(os.path.join(GOLDEN, "utt_sa1_clean.npz"))["samples"]
    pairs = []
    for k, (a, b) in enumerate(((0, n.size), (4000, 4000 + 30000))):
        pn, pc = str(tmp_path / ("noisy%d.npz" % k)), str(tmp_path / ("clean%d.npz" % k))
        np.savez(pn, samples=n[a:b], fs=np.array(16000))
        np.savez(pc, samples=c[a:b + 500], fs=np.array(16000))                  # the clean file is longer: cropped
        pairs.append((pn, pc))
    listing = tmp_path / "pairs.txt"
    listing.write_text("".join("%s %s\n" % p for p in pairs))
    return pairs, str(listing)


def test_wav_pairs_step_matches_single_utterance_chain(tmp_path):
    from avvad import train as TR
    from packages.processing.stft import stft_pytorch
    from packages.processing.target import clean_speech_IBM, clean_speech_VAD
    pairs, listing = pair_files(tmp_path)
    ds = TR.WavPairs(listing)
    assert len(ds) == 2 and ds.pairs == pairs
    batch = TR.WavPairs.collate([ds[0], ds[1]])
    for y_dim in (1, 513):
        lengths, x, y = TR.wav_pair_step(batch, torch.device(DEV), TR.labels_for_ydim(y_dim))
        assert y.shape[-1] == y_dim and x.shape[:2] == y.shape[:2]
        for i, (pn, pc) in enumerate(pairs):
            noisy, _ = TR.load_waveform(pn)
            clean, _ = TR.load_waveform(pc)
            clean = clean[:noisy.numel()]
            T = int(lengths[i])
            feats = TR.audio_features(noisy.to(DEV), std_norm=False)
            assert feats.shape[1] == T
            # the same log power up to the DFT GEMM's summation order (its stream-K split follows the row count): compare
            # powers against the utterance's largest
            p1, p2 = x[i, :T].double().exp(), feats[0].double().exp()
            assert (p1 - p2).abs().max() <= 1e-5 * p2.max()
            c = torch.from_numpy(clean.numpy() / np.max(np.abs(clean.numpy()))).to(DEV)
            if y_dim == 1:
                assert torch.equal(y[i, :T, 0], clean_speech_VAD(c, wlen_sec=64e-3, center=False)[0])
            else:
                ref = clean_speech_IBM(stft_pytorch(c, wlen_sec=64e-3, center=False)).T
                diff = (y[i, :T] != ref).cpu().numpy().T
                if diff.any():
                    _, mag, M, tau = R.ibm_parts(spectrum64(c.cpu().numpy()), 1e-8, 50)
                    assert not (diff & ~ibm_band(mag, M, tau)).any()
            assert not y[i, T:].any()
    with pytest.raises(ValueError):
        TR.labels_for_ydim(3)


def test_train_and_evaluate_on_wav_pairs(tmp_path, capsys):
    from avvad import train as TR
    from packages.models.Audio_Net import DeepVAD_audio
    from packages.processing.target import clean_speech_VAD
    pairs, listing = pair_files(tmp_path)
    for y_dim in (1, 513):
        model = TR.train_main("audio", lambda: DeepVAD_audio(1, 16, y_dim), "wp%d" % y_dim, epochs=1, batch_size=2,
                              out_dir=str(tmp_path / ("m%d" % y_dim)), wav_pairs=listing)
        out = capsys.readouterr().out
        assert "Epoch:  1" in out and "nan" not in out.lower()
        assert all(torch.isfinite(p).all() for p in model.parameters())
    with pytest.raises(ValueError):
        TR.train_main("audio", lambda: DeepVAD_audio(1, 16, 1), "wpw", waveform=True, wav_pairs=listing,
                      out_dir=str(tmp_path / "w"))
    with pytest.raises(ValueError):
        TR.train_main("audio", lambda: DeepVAD_audio(1, 16, 2), "wp2", wav_pairs=listing, out_dir=str(tmp_path / "y2"))
    ev = tmp_path / "eval"
    TR.evaluate_main("audio", lambda: DeepVAD_audio(1, 16, 1), out_dir=str(ev), wav_list=[p[0] for p in pairs],
                     clean_of=dict(pairs))
    for pn, pc in pairs:
        noisy, _ = TR.load_waveform(pn)
        clean, _ = TR.load_waveform(pc)
        clean = clean[:noisy.numel()].numpy()
        c = torch.from_numpy(clean / np.max(np.abs(clean))).to(DEV)
        want = clean_speech_VAD(c, wlen_sec=64e-3, center=False).int().cpu()
        base = str(ev / os.path.splitext(os.path.basename(pn))[0])
        got = torch.load(base + "_label.pt", weights_only=True)
        hard = torch.load(base + "_y_hat_hard.pt", weights_only=True)
        assert torch.equal(got, want) and hard.shape == got.shape
    capsys.readouterr()
    TR.metrics_main(str(ev))
    table = capsys.readouterr().out
    print(table)
    assert "f1" in table.lower()
