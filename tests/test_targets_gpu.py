"""GPU tests of the training labels (csrc/target.hip through avvad.ops and the drop-in packages/processing/target.py):
against the reference's results (tests/golden/targets.npz) outside the stated rounding bands, against the float64
restatement (tests/target_ref.py), ragged batches against single calls, degenerate inputs, reproducibility, every
framing form and every loop of the label kernels past its first trip, and the real-audio data path of the train /
evaluate loops."""
import os

import numpy as np
import pytest
import torch

import target_ref as R
from conftest import GOLDEN, load_golden
from test_targets_cpu import CFGS, IBM_DELTA, ibm_band, ibm_case, sa1, spectrum_case, vad_band

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


# ------------------------------------------------------------------ past one loop trip and in every framing form
# The cases come from tests/target_ref.py; tests/test_targets_cpu.py asserts from the float64 reference that each one can
# fail: the ones shares, the empty tie bands, and the labels a minimum or maximum lost between trips would change.
def run_vad_case(name, mode=None):
    """one call of ops.speech_targets for the case; every row against vad_energy of that row alone, exact outside TIE"""
    from avvad import ops
    case = R.vad_cases()[name]
    wave, lens = R.batch_of(case["rows"])
    frames, out = ops.speech_targets(torch.from_numpy(wave).to(DEV), lens, "vad_labels", center=mode is not None,
                                     pad_mode=mode or "reflect", **R.framing(case["n_fft"], case["hop"]))
    assert frames.tolist() == case["T"] and out.shape == (len(lens), max(case["T"]), 1)
    got = out.cpu().numpy()[:, :, 0]
    assert np.isin(got, (0.0, 1.0)).all()
    for b, T in enumerate(case["T"]):
        E, c = R.vad_reference(case, b, mode)
        thr = c * E.min()
        tie = np.abs(E - thr) <= TIE * thr
        bad = (got[b, :T].astype(bool) != (E > thr)) & ~tie
        print("VAD %s %s row %d: T %d, %d frames excluded, %d differ" % (name, mode or "", b, T, tie.sum(), bad.sum()))
        assert not bad.any(), (name, mode, b, np.flatnonzero(bad)[:8])
        assert not got[b, T:].any(), (name, mode, b)


def test_vad_vector_store_past_1024_frames():
    """vad_decide at T = 1028: five trips of the minimum loop (256 frames a trip; the quietest frame lies in the fourth),
    two of the float4 store loop (1024 frames a trip).  segment_energy, hop-block form (R = 4, seg = 16): 33 workgroups
    of 32 segments, eight trips of each wave's segment loop, one of the k loop."""
    run_vad_case("vec_store_T1028")


def test_vad_scalar_store_with_the_minimum_in_the_last_quad():
    """vad_decide at T = 1027 (T % 4 != 0): five trips of the minimum loop and five of the scalar store loop; the quietest
    frame is the last: the fifth trip, which has three live threads, reads it, and the fifth store trip writes 1, 1, 0."""
    run_vad_case("scalar_store_T1027")


@pytest.mark.parametrize("name", ["whole_frame_vec", "whole_frame_scalar"])
def test_vad_whole_frame_form(name):
    """segment_energy in the whole-frame form (n_fft = 1024, hop = 307: R = 1, seg = 1024, stride 307): four trips of the k
    loop per frame, eight of the segment loop; with L % 4 == 0 the float4 loads are on and taken by every fourth frame
    only ((s0 & 3) == 0), with L % 4 != 0 every load is scalar.  vad_decide at T = 257: two trips of the minimum loop.
    Every frame's label is decided by one loud sample, which lies in another k trip from frame to frame and, for every
    eighth frame, in the last three samples that a load from an aligned address would miss."""
    run_vad_case(name)


@pytest.mark.parametrize("name", ["ragged_quad_whole_frame", "ragged_quad_hop_block"])
def test_vad_guarded_last_quad(name):
    """segment_energy with seg % 4 == 2: the last quad of a segment is loaded sample by sample behind the k + q < seg
    guards, in the whole-frame form (seg = n_fft = 1002, four k trips) and in the hop-block form (n_fft = 1000: R = 4,
    seg = hop = 250, one k trip).  vad_decide: one trip.  Loud single samples sit in the two guarded places of a segment
    and in the two just behind it: dropping the former or adding the latter changes labels."""
    run_vad_case(name)


def test_vad_hop_block_form_with_a_segment_past_256_samples():
    """segment_energy in the hop-block form with seg = hop = 512 (n_fft = 1024, R = 2): two trips of the k loop;
    vad_decide adds two blocks per frame, one trip.  Loud single samples lie in the second half of some blocks and in the
    first half of others, so either k trip alone gives other labels."""
    run_vad_case("hop_block_seg512")


@pytest.mark.parametrize("mode", ["reflect", "constant"])
def test_vad_centred_ragged_batch(mode):
    """segment_energy through sample_at on a centred ragged batch (n_fft = 64, hop 16, three rows; nseg = 130 for the
    longest: five workgroups, eight trips of each wave's segment loop, one of the k loop; vad_decide: one trip): the
    reflection point 2 (n - 1) - s is each row's own, row 0 fills the pitch so its end pad and part of its reflection
    lie past the row (n > nread), rows 1 and 2 differ in the end-pad decision; 'constant' is the zero-padding mode.
    Single loud samples decide the first and last frames: the two modes, a reflection about another row's end or about
    the length without the end pad, and a read past the row's width each give other labels (test_targets_cpu.py)."""
    run_vad_case("centred_ragged", mode)


def test_vad_long_and_short_rows_in_one_call():
    """vad_decide with T = 1028 and T = 185 in one launch, 100x apart in level: the long row's workgroup runs five trips
    of the minimum loop (its quietest frame in the fourth), the short row's one; the store loops run to Tp = 1028 for
    both (two float4 trips), zeros past the short row's frames."""
    run_vad_case("long_and_short")


def test_ibm_batch_past_one_grid_stride_trip():
    """ibm_mask on B * T * 513 = 4 * 4101 * 513 = 8,415,252 outputs: two trips of the grid-stride loop (8192 workgroups
    x 256 threads x 4 outputs a trip), the second in live frames of the last row; T odd, so quads cross rows and
    utterances.  spectrum_max: every row ends in a partial slab (T_b % 8 != 0), and rows 1 and 3 have their loudest bin
    there.  robust: segment_energy (R = 4, seg = 256, one k trip) and vad_decide at T = 4101 (17 trips of the minimum loop
    and of the scalar store loop for the longest row)."""
    from avvad import ops
    rows, ref = ibm_case()
    wave, lens = R.batch_of(rows)
    w = torch.from_numpy(wave).to(DEV)
    frames, plain = ops.speech_targets(w, lens, "ibm_labels")
    _, robust = ops.speech_targets(w, lens, "ibm_labels", robust=True)
    _, vad = ops.speech_targets(w, lens, "vad_labels")
    Tp = max(R.IBM_FRAMES)
    assert frames.tolist() == list(R.IBM_FRAMES) and plain.shape == robust.shape == (len(rows), Tp, 513) and vad.shape == (len(rows), Tp, 1)
    assert torch.equal(robust, plain * vad)
    got, v = plain.cpu().numpy(), vad.cpu().numpy()[:, :, 0]
    assert np.isin(got, (0.0, 1.0)).all()
    for b, T in enumerate(R.IBM_FRAMES):
        bad = (got[b, :T].astype(bool) != ref[b]["mask"]) & ~ref[b]["band"]
        print("IBM batch row %d: T %d, %d of %d bins excluded (delta %.0e), %d differ"
              % (b, T, ref[b]["band"].sum(), bad.size, IBM_DELTA, bad.sum()))
        assert not bad.any(), (b, np.argwhere(bad)[:8])
        assert not got[b, T:].any() and not v[b, T:].any(), b
        E, thr = ref[b]["E"], ref[b]["vad_thr"]
        tie = np.abs(E - thr) <= TIE * thr
        assert np.array_equal(v[b, :T].astype(bool)[~tie], (E > thr)[~tie]), b


def test_ibm_from_spectrum_past_one_trip_in_every_layout():
    """spectrum_max_strided on 513 x 8200 = 4,206,600 bins: 17 trips of the grid-stride loop (1024 workgroups x 256
    threads a trip), the maximum in the thirteenth; ibm_mask_strided: two trips (4096 workgroups x 256 threads x 4 outputs
    a trip).  Four layouts, each without and with a vad vector, against the kernel's arithmetic restated in float64."""
    from avvad import ops
    S, vad, mask, undecided = spectrum_case()
    F, T = S.shape
    Sd = torch.from_numpy(S).to(DEV)
    vd = torch.from_numpy(vad).to(DEV)

    def layouts():
        yield "complex", Sd, None
        yield "legacy view", torch.view_as_real(Sd), (2 * T, 2, 1)
        yield "transposed storage", torch.view_as_real(Sd.T.contiguous()).permute(1, 0, 2), (2, 2 * F, 1)
        wide = torch.full((F, T + 7), float("nan"), dtype=torch.complex64, device=DEV)
        wide[:, 3:3 + T] = Sd
        yield "column slice", wide[:, 3:3 + T], None
    keep = ~undecided
    for name, spec, strides in layouts():
        if strides:
            assert spec.stride() == strides, name
        for with_vad in (False, True):
            got = ops.ibm_from_spectrum(spec, vad=vd if with_vad else None).cpu().numpy()
            want = mask & (vad != 0)[None, :] if with_vad else mask
            bad = (got != want.astype(np.float32)) & keep
            print("IBM from a spectrum, %s%s: %d of %d bins excluded, %d differ"
                  % (name, " with vad" if with_vad else "", undecided.sum(), got.size, bad.sum()))
            assert got.shape == (F, T) and not bad.any(), (name, with_vad, np.argwhere(bad)[:8])
        del spec


def test_a_row_shorter_than_a_frame_is_refused():
    """ops.target_frames raises AvvadError for such a row, so speech_targets returns before any launch"""
    from avvad import ops
    from avvad._lib import AvvadError
    wave = torch.zeros(2, 5000, device=DEV)
    for labels in ("vad_labels", "ibm_labels"):
        with pytest.raises(AvvadError, match="shorter than one"):
            ops.speech_targets(wave, [5000, 500], labels)
    with pytest.raises(AvvadError, match="shorter than one"):
        ops.speech_targets(wave, [5000, 600], "vad_labels", pad_at_end=False)


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
