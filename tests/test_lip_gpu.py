"""GPU tests of the video front-end (csrc/lip.hip through avvad.ops / avvad.train) against the float64 restatement
tests/lip_ref.py: unquantised and quantised frames, the frame map and lengths of ragged batches, constant utterances, the
fused statistics and standardisation, and video / AV training and scoring from files.

Measured on the MI355X (40-frame synthetic utterance): see the docstrings of the first two tests."""
import os

import numpy as np
import pytest
import torch

import lip_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NPIX = 67 * 67
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def float32_deviation(coef):
    """Largest per-pixel deviation from the float64 restatement of a numpy float32 evaluation of the same formula on
    the same input: what fp32 arithmetic costs, whatever the device."""
    c32 = np.asarray(coef, np.float32).reshape(-1, 67, 67)
    C32 = R.dct_matrix().astype(np.float32)
    A = np.einsum("ia,nab,jb->nij", C32, c32, C32)
    assert A.dtype == np.float32
    rng = (A.max(axis=(-2, -1)) - A.min(axis=(-2, -1))).max()
    V = (A - A.min()) / rng * np.float32(255.0)
    assert V.dtype == np.float32
    return float(np.abs(R.rot90_3(V) - R.frames(coef, quantize=False)).max())


def tolerance(coef):
    """4 x the float32 numpy deviation (a different order of the 67-term sums), never above 0.01 level"""
    return min(4.0 * float32_deviation(coef), 0.01)


def decode(coef, n_in, **kw):
    from avvad import ops
    c = coef if isinstance(coef, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(coef))
    return ops.lip_decode(c.to(DEV), n_in, **kw)


def test_unquantised_frames_against_float64():
    """MI355X, 40 synthetic frames: largest deviation 1.55e-4 level against a tolerance of 4.28e-3 (4 x the 1.07e-3 of
    the numpy float32 evaluation)."""
    coef = R.synthetic_coef(40, seed=0)
    ref = R.decode(coef, quantize=False)
    tol = tolerance(coef)
    video, lens = decode(coef, [40], quantize=False)
    assert lens.tolist() == [ref.shape[0]] == [83] and tuple(video.shape) == (1, 83, 67, 67)
    got = video[0].cpu().numpy().astype(np.float64)
    err = np.abs(got - ref).max()
    print("unquantised: max |gpu - float64| = %.3e level, tolerance %.3e (float32 numpy %.3e); max value %.6f"
          % (err, tol, float32_deviation(coef), got.max()))
    assert 0 < tol <= 0.01
    assert err <= tol
    assert ref.max() > 255.0 and got.max() > 255.0               # unclipped


def test_quantised_levels_against_float64():
    """MI355X, 40 synthetic frames: 0.0005 % of the pixels differ from the reference's level, all of them excused (the
    reference's value within the tolerance of an integer, difference exactly 1); 0.86 % of the pixels are excusable."""
    coef = R.synthetic_coef(40, seed=0)
    tol = tolerance(coef)
    exact = R.decode(coef, quantize=False)
    ref = R.quantise(exact)
    video, _ = decode(coef, [40])
    got = video[0].cpu().numpy().astype(np.float64)
    assert np.array_equal(got, np.trunc(got)) and got.min() >= 0 and got.max() <= 255
    near = np.abs(exact - np.rint(exact)) <= tol                  # the clip bounds 0 and 255 are integers too
    excusable = float(near.mean())
    differ = got != ref
    print("quantised: %.4f %% of the pixels differ, %.4f %% excusable at tolerance %.3e" % (100 * differ.mean(), 100 * excusable, tol))
    assert excusable <= 0.03 and differ.mean() <= 0.03          # a test that excuses more than 3 % fails whatever the values
    assert np.all(near[differ])
    assert np.all(np.abs(got - ref)[differ] == 1.0)


@pytest.mark.parametrize("quantize", [True, False])
def test_ragged_batch_equals_single_utterances(quantize):
    from avvad import ops
    n_in = [13, 0, 192, 1, 2]
    utts = [R.synthetic_coef(n, seed=3 + b, scale=1.0 + 11.0 * b) for b, n in enumerate(n_in)]
    t_video = [ops.lip_out_frames(n) for n in n_in]
    assert t_video == [27, 0, 400, 2, 4]
    n_out = [20, 5, 500, 2, 3]                                   # below, (empty), above, equal, below
    want = [min(a, b) for a, b in zip(t_video, n_out)]
    packed = np.concatenate(utts, axis=0)
    padded = np.zeros((5, 192, NPIX), np.float32)
    for b, u in enumerate(utts):
        padded[b, :n_in[b]] = u
        padded[b, n_in[b]:] = 1e6 * (b + 1)                      # what lies behind an utterance is never read
    singles = []
    for b, u in enumerate(utts):
        v, l = decode(u, [n_in[b]], n_out=[n_out[b]], quantize=quantize)
        assert l.tolist() == [want[b]] and tuple(v.shape) == (1, want[b], 67, 67)
        singles.append(v[0])
    for coef in (packed, padded):
        video, lens = decode(coef, n_in, n_out=n_out, quantize=quantize)
        assert lens.tolist() == want and tuple(video.shape) == (5, max(want), 67, 67)
        for b in range(5):
            assert torch.equal(video[b, :want[b]], singles[b])
            assert not video[b, want[b]:].any()                  # padded frames are zero
    # uncapped, and the frame map itself: output frame k is input frame map[k], exactly
    video, lens = decode(packed, n_in, quantize=quantize)
    assert lens.tolist() == t_video
    for b in (0, 2, 4):
        per_input = decode(utts[b], [n_in[b]], quantize=quantize, fs=16000, hop=160, fps_in=100)[0][0]   # p / q = 1: one each
        assert per_input.shape[0] == n_in[b]
        assert torch.equal(video[b, :t_video[b]], per_input[torch.from_numpy(R.frame_map(n_in[b])).to(DEV)])
        ref = R.decode(utts[b], quantize=quantize)
        assert np.abs(video[b, :t_video[b]].cpu().numpy() - ref).max() <= (1.0 if quantize else tolerance(utts[b]))
    assert not video[1].any() and not video[3, 2:].any()


def test_constant_utterances_are_written_as_zero():
    flat = np.zeros((6, NPIX), np.float32)
    flat[:, 0] = 5.0                                             # the DC term alone: every frame constant, range 0
    video, lens = decode(flat, [6])
    assert lens.tolist() == [13] and torch.isfinite(video).all() and not video.any()
    video, _ = decode(np.zeros((3, NPIX), np.float32), [3], quantize=False)
    assert torch.isfinite(video).all() and not video.any()
    # a constant utterance between two ordinary ones: no reduction crosses an utterance
    a, c = R.synthetic_coef(7, seed=1), R.synthetic_coef(9, seed=2, scale=3.0)
    video, lens = decode(np.concatenate([a, flat, c]), [7, 6, 9])
    assert lens.tolist() == [15, 13, 19]
    assert not video[1].any() and torch.isfinite(video).all()
    assert torch.equal(video[0, :15], decode(a, [7])[0][0]) and torch.equal(video[2, :19], decode(c, [9])[0][0])
    assert video[0].max() == 255 and video[2].max() == 255


def test_fused_statistics_are_exact_and_reproducible(lib_options):
    from avvad import ops
    n_in = [13, 40, 0, 25]
    n_out = [27, 60, 4, 100]
    coef = np.concatenate([R.synthetic_coef(n, seed=5 + b, scale=2.0 + b) for b, n in enumerate(n_in)])
    acc = ops.stats_new(1, DEV)
    video, lens = decode(coef, n_in, n_out=n_out, acc=acc)
    assert lens.tolist() == [27, 60, 0, 52]
    v = video.cpu().numpy().astype(np.float64)
    vals = np.concatenate([v[b, :n].reshape(-1) for b, n in enumerate(lens.tolist())])
    host = [float(vals.sum()), float((vals * vals).sum()), float(vals.size)]      # integers below 2^53: exact
    assert vals.size == sum(lens.tolist()) * NPIX and host[1] < 2.0 ** 53
    assert acc.tolist() == host
    other = ops.accumulate_stats(ops.stats_new(1, DEV), video.view(4, -1, NPIX), lens, nstat=1)
    assert torch.equal(acc, other)
    # accumulators add: a second batch into the same one
    decode(coef, n_in, acc=acc)
    full = decode(coef, n_in)[0].cpu().numpy().astype(np.float64)
    assert acc.tolist() == [host[0] + full.sum(), host[1] + (full * full).sum(), host[2] + sum(ops.lip_out_frames(n) for n in n_in) * NPIX]
    # unquantised: two runs and a CU-capped run give the same bits, frames and sums
    a1, a2, a3 = (ops.stats_new(1, DEV) for _ in range(3))
    v1, _ = decode(coef, n_in, n_out=n_out, quantize=False, acc=a1)
    v2, _ = decode(coef, n_in, n_out=n_out, quantize=False, acc=a2)
    lib_options("max_cus", 8)
    v3, _ = decode(coef, n_in, n_out=n_out, quantize=False, acc=a3)
    assert torch.equal(v1, v2) and torch.equal(v1, v3) and torch.equal(a1, a2) and torch.equal(a1, a3)
    d = v1.double()
    assert abs(float(a1[0]) - float(d.sum())) <= 1e-9 * float(d.sum()) and float(a1[2]) == host[2]
    mean, std = ops.finalize_stats(acc)
    n = acc[2].item()
    mu = acc[0].item() / n
    assert abs(mean.item() - mu) <= 1e-6 * mu and abs(std.item() - np.sqrt((acc[1].item() - n * mu * mu) / (n - 1))) <= 1e-5 * std.item()


def test_fused_standardisation_equals_stats_video():
    from avvad import ops
    from avvad.train import Stats
    n_in = [21, 8]
    coef = np.concatenate([R.synthetic_coef(n, seed=9 + b) for b, n in enumerate(n_in)])
    st = Stats(video_mean=np.array([[97.25]], np.float32), video_std=np.array([[61.5]], np.float32))
    acc0, acc1 = ops.stats_new(1, DEV), ops.stats_new(1, DEV)
    plain, lens = decode(coef, n_in, n_out=[40, 17], acc=acc0)
    fused, lens1 = decode(coef, n_in, n_out=[40, 17], acc=acc1, mean=st.get("video_mean", torch.device(DEV)),
                          std=st.get("video_std", torch.device(DEV)), eps=st.eps)
    assert lens.tolist() == lens1.tolist() == [40, 17]
    assert torch.equal(acc0, acc1)                               # the statistics are of the unstandardised values
    want = st.video(plain)
    for b, n in enumerate(lens.tolist()):
        a, w = fused[b, :n], want[b, :n]
        # one subtract and one divide in float32, each correctly rounded, on both sides: at most an ulp of the quotient apart
        assert torch.all((a - w).abs() <= 2.0 ** -23 * w.abs().clamp_min(2.0 ** -126))
        assert not fused[b, n:].any()                            # padding stays zero, it is not standardised
    with pytest.raises(Exception):
        decode(coef, n_in, mean=st.get("video_mean", torch.device(DEV)))


def av_fixture(tmp_path, n_utts=3):
    """(noisy, clean, coefficients) files: the fixture utterance and crops of it, with synthetic lip coefficients whose
    frame count follows the audio's duration at 30 frames/s."""
    n = np.load(os.path.join(GOLDEN, "utt_sa1.npz"))["samples"]
    c = np.load(os.path.join(GOLDEN, "utt_sa1_clean.npz"))["samples"]
    triples = []
    for k, cut in enumerate((len(n), 30000, 36000)[:n_utts]):
        pn, pc, pv = (str(tmp_path / (name % k)) for name in ("noisy%d.npz", "clean%d.npz", "lips%d.npy"))
        np.savez(pn, samples=n[:cut], fs=np.array(16000))
        np.savez(pc, samples=c[:cut], fs=np.array(16000))
        np.save(pv, R.synthetic_coef(int(round(cut / 16000 * 30)), seed=20 + k).astype(np.float64))   # doubles, as the .mat files hold
        triples.append((pn, pc, pv))
    listing = tmp_path / "av.txt"
    listing.write_text("".join("%s %s %s\n" % t for t in triples))
    return triples, str(listing)


def test_av_file_step_matches_the_single_utterance_chains(tmp_path):
    from avvad import ops
    from avvad import train as TR
    triples, listing = av_fixture(tmp_path)
    dev = torch.device(DEV)
    ds = TR.AVFiles(listing)
    assert len(ds) == 3 and ds[0][3].dtype == torch.float32
    batch = TR.AVFiles.collate([ds[i] for i in range(3)])
    lengths, x, video, y = TR.av_file_step(batch, dev, "vad_labels")
    frames, x0, y0 = TR.wav_pair_step(batch[:3], dev, "vad_labels")
    assert torch.equal(x, x0) and torch.equal(y, y0)
    assert video.shape[:2] == x.shape[:2] and tuple(video.shape[2:]) == (67, 67)
    for b in range(3):
        coef = np.load(triples[b][2])
        t_label = int(frames[b])
        assert int(lengths[b]) == min(t_label, ops.lip_out_frames(coef.shape[0])) == t_label    # the video is capped to the labels
        ref = R.decode(coef.astype(np.float32), n_out=t_label)
        got = video[b, :t_label].cpu().numpy()
        assert np.abs(got - ref).max() <= 1.0 and (got != ref).mean() <= 0.03
        assert not video[b, t_label:].any()
    from packages.processing.video import decode_ntcd_frames
    one = decode_ntcd_frames(np.load(triples[1][2]), n_label_frames=int(frames[1]))
    assert isinstance(one, np.ndarray) and one.dtype == np.float32
    assert np.array_equal(one, video[1, :int(frames[1])].cpu().numpy())
    on_gpu = decode_ntcd_frames(torch.from_numpy(np.load(triples[1][2])).to(dev))
    assert on_gpu.is_cuda and on_gpu.shape[0] == ops.lip_out_frames(np.load(triples[1][2]).shape[0])


def test_train_and_evaluate_from_av_files(tmp_path, capsys):
    from avvad import ops
    from avvad import train as TR
    from packages.models.AV_Net import DeepVAD_AV
    from packages.models.Video_Net import DeepVAD_video
    triples, listing = av_fixture(tmp_path)
    dev = torch.device(DEV)
    makers = {"video": lambda: DeepVAD_video(1, 16, 1), "AV": lambda: DeepVAD_AV(1, 16, 1)}
    for kind, make in makers.items():
        out = str(tmp_path / ("model_" + kind))
        TR.train_main(kind, make, "lip_" + kind, epochs=6, batch_size=3, lr=1e-3, out_dir=out, av_files=listing, compute_stats=True)
        log = capsys.readouterr().out
        losses = [float(line.split("train loss")[1].split()[0]) for line in log.splitlines() if "====> Epoch" in line]
        print(kind, "train losses", losses)
        assert len(losses) == 6 and all(np.isfinite(losses)) and losses[-1] < losses[0]
        assert "Train-set statistics over 3 utterances" in log
        st = TR.Stats.load(out)
        assert st._raw["video_mean"].shape == st._raw["video_std"].shape == (1, 1) and st._raw["audio_mean"].shape == (513, 1)
        # the stored scalars against a host float64 reduction of the decoded frames (each capped to its label count)
        vals = []
        for pn, pc, pv in triples:
            n_label = ops.target_frames(len(np.load(pn)["samples"]))[1]
            v, l = decode(np.load(pv).astype(np.float32), [np.load(pv).shape[0]], n_out=[n_label])
            vals.append(v[0, :int(l[0])].cpu().numpy().astype(np.float64).reshape(-1))
        vals = np.concatenate(vals)
        assert np.float32(vals.mean()) == st._raw["video_mean"][0, 0]
        assert abs(float(st._raw["video_std"][0, 0]) - vals.std(ddof=1)) <= 1e-6 * vals.std(ddof=1)
        ck = sorted(f for f in os.listdir(out) if f.endswith(".pt"))[-1]
        ev = str(tmp_path / ("eval_" + kind))
        TR.evaluate_main(kind, make, checkpoint=os.path.join(out, ck), out_dir=ev, av_files=listing, stats=st)
        soft = sorted(f for f in os.listdir(ev) if f.endswith("_y_hat_soft.pt"))
        assert len(soft) == 3 and len([f for f in os.listdir(ev) if f.endswith("_y_hat_hard.pt")]) == 3
        s0 = torch.load(os.path.join(ev, soft[0]), weights_only=True)
        lab = torch.load(os.path.join(ev, soft[0].replace("_y_hat_soft", "_label")), weights_only=True)
        assert s0.shape == lab.shape and torch.isfinite(s0).all()
    # what was refused stays refused, and the new argument refuses what it cannot do
    with pytest.raises(ValueError):
        TR.train_main("audio", makers["video"], "x", av_files=listing, out_dir=str(tmp_path / "x"))
    with pytest.raises(ValueError):
        TR.train_main("video", makers["video"], "x", wav_pairs=[t[:2] for t in triples], out_dir=str(tmp_path / "x"))
    with pytest.raises(ValueError):
        TR.evaluate_main("video", makers["video"], out_dir=str(tmp_path / "x"), wav_list=[t[0] for t in triples])
