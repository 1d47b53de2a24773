"""GPU tests of the video front-end (csrc/lip.hip through avvad.ops / avvad.train) against the float64 restatement
tests/lip_ref.py: unquantised and quantised frames, the frame map and lengths of ragged batches, constant utterances, the
fused statistics and standardisation, and video / AV training and scoring from files.

Measured on the MI355X (40-frame synthetic utterance): see the docstrings of the first two tests.

Past one loop trip (the second half of the file; inputs and oracles in tests/lip_ref.py, their mutants in
tests/test_lip_cpu.py):
* a one-hot utterance -- one nonzero coefficient per frame, so every pixel is ONE product of two table entries and no
  summation order enters -- covering every row and column, all pairs of the MFMA tile edges and the DC frame, staged from
  all four alignments packed and padded: held to ``lip_ref.onehot_bound``, 1.368e-4 level, derived by counting roundings
  (observed on the MI355X: 2.39e-5, the value of the float32 numpy stand-in), the same bits under a cap of 4 CUs (48
  trips with prefetch), quantised levels exact outside the bound;
* 600 frames with the minimum in frame 300 and the largest range in frame 550 (lip_utt's ``i += 256``; observed 2.48e-4
  against a tolerance of 9.11e-4);
* B = 35 utterances of 0..130 frames and B = 1030 of one or two with ``acc=`` (lip_add's wave, lane and count loops, a
  grid of one workgroup per utterance): sums and pixel count equal to the host's integers;
* B = 128 utterances of 9..13 frames (two workgroups per utterance, two ragged trips) against float64 (observed 0.29 of
  the tolerance);
* 25, 50, 100 and 125 input frames/s at hop 256: the frame map bit for bit, and where frames get no slot (p < q) the
  minimum and the largest range lie in such frames.
These use ``lip_ref.tolerance``: the rule of ``tolerance`` below with the float32 evaluation written out term by term
(the same arithmetic on every host, milliseconds per frame); on the 40-frame utterance it is 6.7e-4 against 4.28e-3."""
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


# ------------------------------------------------------------------------------------------ past one loop trip
def log_line(msg):
    """print and append to the parity log of tests/test_gpu_parity.py"""
    from test_gpu_parity import OUT
    print(msg)
    try:
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, "parity.log"), "a") as f:
            f.write(msg + "\n")
    except OSError:
        pass


def check_quantised(got, exact, tol, what):
    """The excuse rule of test_quantised_levels_against_float64: integer levels in 0..255; a pixel may differ from the
    reference's level, by exactly 1, only where the float64 value lies within ``tol`` of an integer; a test that excuses
    more than 3 % fails whatever the values."""
    ref = R.quantise(exact)
    assert got.shape == ref.shape and np.array_equal(got, np.trunc(got)) and got.min() >= 0 and got.max() <= 255
    near = np.abs(exact - np.rint(exact)) <= tol
    differ = got != ref
    print("%s: %.4f %% of the pixels differ, %.4f %% excusable at tolerance %.3e" % (what, 100 * differ.mean(), 100 * near.mean(), np.max(tol)))
    assert near.mean() <= 0.03 and differ.mean() <= 0.03
    assert np.all(near[differ])
    assert np.all(np.abs(got - ref)[differ] == 1.0)


def host_sums(video, lens):
    """[sum, sumsq, count] of the written frames in float64 on the host: exact for quantised frames (integers, < 2^53)"""
    v = video.cpu().numpy().astype(np.float64)
    vals = np.concatenate([v[b, :n].reshape(-1) for b, n in enumerate(lens)])
    host = [float(vals.sum()), float((vals * vals).sum()), float(vals.size)]
    assert host[1] < 2.0 ** 53
    return host


def onehot_batches():
    """the one-hot utterance four times, packed (starts 0, 189, 378, 567) and padded to a pitch of 191 frames (starts 0,
    191, 382, 573): every frame is staged from all four alignments of ``load_raw``, behind nonzero starts"""
    coef, pairs, amp = R.onehot_coef()
    N = coef.shape[0]
    packed = np.concatenate([coef] * 4)
    padded = np.full((4, N + 2, NPIX), 1e6, np.float32)          # what lies behind an utterance is never read
    padded[:, :N] = coef
    assert sorted(s & 3 for s in (0, N, 2 * N, 3 * N)) == sorted(s & 3 for s in (0, N + 2, 2 * N + 4, 3 * N + 6)) == [0, 1, 2, 3]
    return (("packed", packed), ("padded", padded)), pairs, amp


def test_onehot_frames_within_the_counted_roundings(lib_options):
    """One nonzero coefficient per frame: every pixel is one product of two table entries, so an index, transpose,
    reversal or pad mistake is an error of order 1 and the float32 error is bounded by counting roundings
    (lip_ref.onehot_bound: 1.368e-4 level).  MI355X: largest deviation 2.4e-5 level, packed and padded alike; the same
    bits under a cap of 4 CUs (one workgroup per utterance, 48 trips with prefetch)."""
    batches, pairs, amp = onehot_batches()
    N = len(pairs)
    exact = R.onehot_frames64(pairs, amp)
    bound = R.onehot_bound(pairs, amp)
    assert 1.0e-4 < bound < 2.0e-4
    videos = {}
    for name, coef in batches:
        video, lens = decode(coef, [N] * 4, quantize=False, **R.ONE)
        assert lens.tolist() == [N] * 4 and tuple(video.shape) == (4, N, 67, 67)
        got = video.cpu().numpy().astype(np.float64)
        err = [float(np.abs(got[b] - exact).max()) for b in range(4)]
        log_line("lip one-hot %-6s max |gpu - float64| = %.3e level (per alignment %s), derived bound %.3e"
                 % (name, max(err), " ".join("%.2e" % e for e in err), bound))
        assert max(err) <= bound
        videos[name] = video
    lib_options("max_cus", 4)
    for name, coef in batches:
        assert torch.equal(decode(coef, [N] * 4, quantize=False, **R.ONE)[0], videos[name])


def test_onehot_levels_are_exact_outside_the_bound():
    """Quantised one-hot frames: every pixel whose float64 value lies farther than the derived bound from an integer has
    exactly the reference's level (0.05 % of the pixels are excusable)."""
    batches, pairs, amp = onehot_batches()
    N = len(pairs)
    exact = R.onehot_frames64(pairs, amp)
    bound = R.onehot_bound(pairs, amp)
    for name, coef in batches:
        video, _ = decode(coef, [N] * 4, **R.ONE)
        got = video.cpu().numpy().astype(np.float64)
        for b in range(4):
            check_quantised(got[b], exact, bound, "one-hot %s, utterance %d" % (name, b))


def test_frame_loop_of_a_long_utterance():
    """600 frames, the global minimum in frame 300 and the largest range in frame 550: lip_utt's loop takes three trips."""
    coef = R.long_utterance()
    exact = R.decode(coef, quantize=False, **R.ONE)
    tol = R.tolerance(coef)
    video, lens = decode(coef, [R.LONG_N], quantize=False, **R.ONE)
    assert lens.tolist() == [R.LONG_N]
    err = np.abs(video[0].cpu().numpy().astype(np.float64) - exact).max()
    log_line("lip 600 frames: max |gpu - float64| = %.3e level, tolerance %.3e" % (err, tol))
    assert 0 < tol <= 0.01 and err <= tol
    video, _ = decode(coef, [R.LONG_N], **R.ONE)
    check_quantised(video[0].cpu().numpy().astype(np.float64), exact, tol, "600 frames")


def test_statistics_add_over_many_utterances_and_frames():
    """B = 35 utterances of 0..130 frames: lip_add's wave loop and lane loop take three trips each.  Quantised levels are
    integers, so the accumulator equals the host's float64 sums and ``ops.accumulate_stats`` bit for bit."""
    from avvad import ops
    n_in = R.stats_add_counts()
    coef = R.batch_of(n_in, seed=41)
    acc = ops.stats_new(1, DEV)
    video, lens = decode(coef, n_in, acc=acc, **R.ONE)
    assert lens.tolist() == n_in and tuple(video.shape) == (35, 130, 67, 67)
    assert acc.tolist() == host_sums(video, n_in)
    other = ops.accumulate_stats(ops.stats_new(1, DEV), video.view(35, -1, NPIX), lens, nstat=1)
    assert torch.equal(acc, other)
    for b in (0, 9, 34):                                         # and the frames are the single utterances'
        assert torch.equal(video[b, :n_in[b]], decode(R.split(coef, n_in)[b], [n_in[b]], **R.ONE)[0][0])
    assert not video[2].any() and not video[1, 3:].any()


def test_count_loop_and_one_workgroup_per_utterance():
    """B = 1030 utterances of one or two frames: the second trip of lip_add's count loop, and 256 / B == 0 workgroups per
    utterance (a grid of one)."""
    from avvad import ops
    n_in = R.count_counts()
    coef = R.batch_of(n_in, seed=43)
    acc = ops.stats_new(1, DEV)
    video, lens = decode(coef, n_in, acc=acc, **R.ONE)
    assert lens.tolist() == n_in and tuple(video.shape) == (1030, 2, 67, 67)
    host = host_sums(video, n_in)
    assert host[2] == sum(n_in) * NPIX and acc.tolist() == host
    utts = R.split(coef, n_in)
    for b in (0, 1, 2, 3, 255, 256, 257, 511, 512, 767, 1023, 1024, 1025, 1027, 1028, 1029):
        single, _ = decode(utts[b], [n_in[b]], **R.ONE)
        assert torch.equal(video[b, :n_in[b]], single[0]) and not video[b, n_in[b]:].any()
        check = R.decode(utts[b], **R.ONE)
        assert np.abs(single[0].cpu().numpy() - check).max() <= 1.0


def test_ragged_utterances_over_two_trips_of_two_workgroups():
    """B = 128 utterances of 9..13 frames, uncapped: lip_frames runs two workgroups per utterance, eight frames per trip,
    two trips with ragged ends -- against the float64 restatement, utterance by utterance."""
    n_in = R.ragged_counts()
    coef = R.batch_of(n_in, seed=47)
    utts = R.split(coef, n_in)
    raw, lens = decode(coef, n_in, quantize=False, **R.ONE)
    lev, _ = decode(coef, n_in, **R.ONE)
    assert lens.tolist() == n_in
    raw, lev = raw.cpu().numpy().astype(np.float64), lev.cpu().numpy().astype(np.float64)
    worst = 0.0
    exacts, tols = [], []
    for b, n in enumerate(n_in):
        exact = R.decode(utts[b], quantize=False, **R.ONE)
        tol = R.tolerance(utts[b])
        err = np.abs(raw[b, :n] - exact).max()
        worst = max(worst, err / tol)
        assert 0 < tol <= 0.01 and err <= tol, (b, err, tol)
        assert not raw[b, n:].any() and not lev[b, n:].any()
        exacts.append(exact), tols.append(np.full(exact.shape, tol))
    log_line("lip 128 ragged utterances: worst |gpu - float64| / tolerance = %.4f" % worst)
    check_quantised(np.concatenate([lev[b, :n] for b, n in enumerate(n_in)]), np.concatenate(exacts), np.concatenate(tols), "128 ragged")


@pytest.mark.parametrize("fps_in", R.RATES)
def test_rates_above_and_below_one(fps_in):
    """hop 256 at 25, 50, 100 and 125 input frames/s (p / q = 5/2, 5/4, 5/8, 1/2): lengths and frame map against
    lip_ref.frame_map through a gather from the 1:1 decode (bit exact).  Below one, frames without an output slot hold the
    utterance's minimum and its largest range: the normalisation must see them, the statistics must not."""
    from avvad import ops
    rate = dict(fs=16000, hop=256, fps_in=fps_in)
    utts = R.rate_utterances(fps_in)
    n_in = [u.shape[0] for u in utts]
    want = [len(R.frame_map(n, hop=256, fps_in=fps_in)) for n in n_in]
    coef = np.concatenate(utts)
    for quantize in (True, False):
        acc = ops.stats_new(1, DEV)
        video, lens = decode(coef, n_in, quantize=quantize, acc=acc, **rate)
        assert lens.tolist() == want and tuple(video.shape) == (2, max(want), 67, 67)
        for b, n in enumerate(n_in):
            one, _ = decode(utts[b], [n], quantize=quantize, **R.ONE)
            fm = torch.from_numpy(R.frame_map(n, hop=256, fps_in=fps_in)).to(DEV)
            assert torch.equal(video[b, :want[b]], one[0][fm]) and not video[b, want[b]:].any()
            exact = R.decode(utts[b], quantize=False, hop=256, fps_in=fps_in)
            got = video[b, :want[b]].cpu().numpy().astype(np.float64)
            tol = R.tolerance(utts[b])
            if quantize:
                check_quantised(got, exact, tol, "%d frames/s, utterance %d" % (fps_in, b))
            else:
                err = np.abs(got - exact).max()
                log_line("lip %3d frames/s utterance %d: max |gpu - float64| = %.3e level, tolerance %.3e" % (fps_in, b, err, tol))
                assert err <= tol
        if quantize:                                             # the sums are of the written frames only
            assert acc.tolist() == host_sums(video, want)
            assert torch.equal(acc, ops.accumulate_stats(ops.stats_new(1, DEV), video.view(2, -1, NPIX), lens, nstat=1))
        else:
            assert float(acc[2]) == sum(want) * NPIX


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
