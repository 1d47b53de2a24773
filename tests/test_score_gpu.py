"""GPU tests of the scores (csrc/scores.hip through avvad.ops, packages.metrics and the evaluators) against the float64
reference tests/score_ref.py.

Tolerance: 1e-6 dB on every ratio.  The closed form's cancellation e.e - a_s e.s loses a factor 10^(R/10) of double's
2^-53 at a ratio of R dB: at 60 dB that is 1e6 * 4.34 * (a few 1e-16) ~ 1e-9 dB, and tests/test_score_cpu.py repeats on
the CPU the sweep that measured 2.9e-9 dB at worst.  The signals are s_hat = 0.7 s + g n + e with g in {1, 0.1, 1e-3} and
e 0, 20 or 40 dB below s, drawn (next seed on a miss, judged by the REFERENCE alone) so that every ratio lies in
[-10, 60] dB.  alpha: 1e-12 relative -- a double dot product's relative error is a few 2^-53 times sum|terms| / |sum|,
and the draw also keeps that condition number of both projections below 1e3.

Past one trip of the finishing kernels: rows of 8, 9, 10, 16 and 18 chunks (``gram_add``'s add_ascending<8>: the unrolled
body once and twice, alone and with a remainder, all six products under third_mode 1 and 2), an 18-chunk row in packets,
B = 70 (the second workgroup of ``gram_finalize``, rows behind 64 in ``gram_add``'s grid), and confusion counts of ragged
batches whose rows hold several chunks next to chunks that exit ((5, 24, 512)) and of 70 rows ((70, 9, 7))."""
import os

import numpy as np
import pytest
import torch

import score_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
TOL_DB = 1e-6
TOL_ALPHA = 1e-12
T_ = torch.from_numpy


def _ops():
    from avvad import ops
    return ops


C = _ops().SCORE_CHUNK

_draw = score_ref.draw           # (s_hat, s, n, ratios, alphas) of length L with the k-th (gain, artefact) pair


def _gpu(*xs):
    return [T_(np.ascontiguousarray(x)).to(DEV) for x in xs]


def _close(what, got, want, tol=TOL_DB):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    print("%s: got %s want %s |d| %s" % (what, got, want, np.abs(got - want)))
    assert np.isfinite(want).all() and np.isfinite(got).all(), what
    assert np.abs(got - want).max() <= tol, what


@pytest.mark.parametrize("k,L", list(enumerate([2, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3])))
def test_length_sweep(k, L):
    ops = _ops()
    e, s, n, want, alpha = _draw(L, k)
    ed, sd, nd = _gpu(e, s, n)
    ratios, a = ops.energy_ratios(ed.view(1, -1), sd.view(1, -1), noise=nd.view(1, -1), return_alpha=True)
    assert ratios.shape == (1, 3) and ratios.dtype == torch.float64 and ratios.is_cuda and a.shape == (1, 2)
    _close("L = %d ratios" % L, ratios[0].cpu().numpy(), want)
    rel = np.abs(a[0].cpu().numpy() - alpha) / np.abs(alpha)
    print("L = %d alpha rel %s" % (L, rel))
    assert rel.max() <= TOL_ALPHA
    # (L,) signals are one row
    assert torch.equal(ops.energy_ratios(ed, sd, noise=nd), ratios)


def test_ragged_batch_reads_nothing_behind_the_lengths():
    """Row 1 is ONE sample: its estimate is a multiple of its reference, so SI-SDR is +inf; the dyadic values make every
    product and quotient exact, and the planes form and the closed form both give (inf, 0 dB, 0 dB) exactly."""
    ops = _ops()
    P = C + 77
    lengths = [P, 1, 300, 0]
    rows = [_draw(P, 4)[:3], (np.float32([0.25]), np.float32([0.5]), np.float32([-0.125])), _draw(300, 7)[:3], None]
    est, ref, noise = (np.full((4, P), NAN, dtype=np.float32) for _ in range(3))
    for b, sig in enumerate(rows):
        if sig is not None:
            est[b, :lengths[b]], ref[b, :lengths[b]], noise[b, :lengths[b]] = sig
    ed, sd, nd = _gpu(est, ref, noise)
    ratios, alpha = ops.energy_ratios(ed, sd, noise=nd, lengths=lengths, return_alpha=True)
    ratios, alpha = ratios.cpu().numpy(), alpha.cpu().numpy()
    print(ratios, alpha)
    for b in (0, 2):
        _close("row %d" % b, ratios[b], score_ref.energy_ratios(*rows[b]))
        assert (np.abs(alpha[b] - score_ref.alphas(*rows[b])) <= TOL_ALPHA * np.abs(alpha[b])).all()
    want1 = np.array(score_ref.energy_ratios(*rows[1]))
    assert want1.tolist() == [np.inf, 0.0, 0.0] and ratios[1, 0] == np.inf
    _close("row 1 (si_sir, si_sar)", ratios[1, 1:], want1[1:])
    assert alpha[1].tolist() == list(score_ref.alphas(*rows[1])) == [0.5, -2.0]
    assert np.isnan(ratios[3]).all() and np.isnan(alpha[3]).all()
    assert not np.isnan(ratios[:3]).any() and not np.isnan(alpha[:3]).any()
    # lengths as a tensor, and beyond the row: clamped to the row
    again = ops.energy_ratios(ed[:1], sd[:1], noise=nd[:1], lengths=torch.LongTensor([P + 1000]))
    assert torch.equal(again.cpu(), T_(ratios[:1]))


def test_third_input_modes():
    ops = _ops()
    L = C + 5
    e, s, n, want, _ = _draw(L, 1)
    x = (s + n).astype(np.float32)                          # the noisy mixture as the file holds it
    ed, sd, nd, xd = _gpu(e, s, n, x)
    want_mix = score_ref.energy_ratios(e, s, x.astype(np.float64) - s.astype(np.float64))
    assert all(-10 <= v <= 60 for v in want_mix)
    got, alpha = ops.energy_ratios(ed, sd, mixture=xd, return_alpha=True)
    _close("mixture", got[0].cpu().numpy(), want_mix)
    a_ref = np.array(score_ref.alphas(e, s, x.astype(np.float64) - s.astype(np.float64)))
    assert (np.abs(alpha[0].cpu().numpy() - a_ref) <= TOL_ALPHA * np.abs(a_ref)).all()
    none, a0 = ops.energy_ratios(ed, sd, return_alpha=True)
    none, a0 = none[0].cpu().numpy(), a0[0].cpu().numpy()
    _close("none: si_sdr", none[:1], want[:1])
    assert np.isnan(none[1:]).all() and np.isnan(a0[1]) and abs(a0[0] - a_ref[0]) <= TOL_ALPHA * abs(a_ref[0])
    with pytest.raises(ops.L.AvvadError, match="not both"):
        ops.energy_ratios(ed, sd, noise=nd, mixture=xd)


def test_row_pitches_are_read_in_place():
    ops = _ops()
    L, B = C + 5, 2
    sig = [_draw(L, 3)[:3], _draw(L, 5)[:3]]
    wide = [torch.full((B, L + pad), NAN, device=DEV) for pad in (9, 3, 14)]
    views = [wide[0][:, 1:1 + L], wide[1][:, :L], wide[2][:, 2:2 + L]]
    for j, v in enumerate(views):
        v.copy_(T_(np.stack([sig[b][j] for b in range(B)])))
        assert not v.is_contiguous() and v.stride() == (wide[j].shape[1], 1)
    got, ga = ops.energy_ratios(views[0], views[1], noise=views[2], return_alpha=True)
    want, wa = ops.energy_ratios(*[v.contiguous() for v in views[:2]], noise=views[2].contiguous(), return_alpha=True)
    assert torch.equal(got, want) and torch.equal(ga, wa)
    for b in range(B):
        _close("row %d" % b, got[b].cpu().numpy(), score_ref.energy_ratios(*sig[b]))
    # a longer clean / noise row: its first L samples count; a last axis that is not unit-stride is copied
    assert torch.equal(ops.energy_ratios(views[0], wide[1], noise=wide[2][:, 2:]), got)
    twice = torch.stack([views[0], views[0]], dim=2)[:, :, 0]
    assert twice.stride(1) == 2 and torch.equal(ops.energy_ratios(twice, views[1], noise=views[2]), got)


def test_packets_add_up_and_repeat_bit_for_bit(lib_options):
    ops = _ops()
    L = 2 * C + 3
    e, s, n, want, _ = _draw(L, 6)
    ed, sd, nd = _gpu(e, s, n)

    def run(cuts):
        acc = ops.score_state(1, DEV)
        edges = [0] + list(cuts) + [L]
        for a, b in zip(edges[:-1], edges[1:]):
            assert ops.score_accumulate(acc, ed[a:b], sd[a:b], noise=nd[a:b]) is acc
        return ops.score_finalize(acc, "noise"), acc.clone()
    splits = {"single": (), "1 | rest": (1,), "C-1 | rest": (C - 1,), "five uneven": (7, C + 1, C + 130, 2 * C - 1)}
    first = {}
    for name, cuts in splits.items():
        first[name] = run(cuts)
        _close("packets %s" % name, first[name][0][0].cpu().numpy(), want)
        again = run(cuts)
        assert torch.equal(again[0], first[name][0]) and torch.equal(again[1], first[name][1]), name
    lib_options("max_cus", 32)
    capped = run(())
    assert torch.equal(capped[0], first["single"][0]) and torch.equal(capped[1], first["single"][1])


def _ragged(rows, P):
    """(est, ref, noise) (B, P) float32 on the GPU from per-row (s_hat, s, n) or None, NaN behind every row's length"""
    planes = [np.full((len(rows), P), NAN, dtype=np.float32) for _ in range(3)]
    for b, sig in enumerate(rows):
        if sig is not None:
            for plane, x in zip(planes, sig):
                plane[b, :x.size] = x
    return _gpu(*planes)


@pytest.mark.parametrize("third", ["noise", "mixture"])
def test_rows_of_eight_to_eighteen_chunks(third):
    """One ragged batch of rows of 8 C, 8 C + 1, 9 C + 5, 16 C and 17 C + 3 samples, NaN behind every length: the sum of a
    row's partials runs its unrolled body once or twice, alone and followed by a remainder of one or two chunks.  Ratios and
    alphas against float64; each row alone (a partial pitch of its own chunk count) gives the batch row's bits; two runs
    give equal bits."""
    ops = _ops()
    lengths = score_ref.many_chunk_lengths(C)
    P = max(lengths) + 77
    rows, want, want_a = [], [], []
    for k, L in enumerate(lengths):
        e, s, n, r, a = _draw(L, k)
        if third == "mixture":
            x, n64 = score_ref.mixture_of(s, n)
            rows.append((e, s, x))
            want.append(score_ref.energy_ratios(e, s, n64))
            want_a.append(score_ref.alphas(e, s, n64))
        else:
            rows.append((e, s, n))
            want.append(r)
            want_a.append(a)
    want, want_a = np.array(want), np.array(want_a)
    assert np.all((want >= -10.0) & (want <= 60.0))
    ed, sd, td = _ragged(rows, P)
    ratios, alpha = ops.energy_ratios(ed, sd, lengths=lengths, return_alpha=True, **{third: td})
    assert ratios.shape == (5, 3) and alpha.shape == (5, 2)
    for b, L in enumerate(lengths):
        _close("%s, row of %d samples" % (third, L), ratios[b].cpu().numpy(), want[b])
        rel = np.abs(alpha[b].cpu().numpy() - want_a[b]) / np.abs(want_a[b])
        print("alpha rel %s" % rel)
        assert rel.max() <= TOL_ALPHA
        one, one_a = ops.energy_ratios(ed[b:b + 1, :L], sd[b:b + 1, :L], return_alpha=True, **{third: td[b:b + 1, :L]})
        _close("%s, the row of %d samples alone" % (third, L), one[0].cpu().numpy(), want[b])
        assert torch.equal(one[0], ratios[b]) and torch.equal(one_a[0], alpha[b]), (third, L)
    again, again_a = ops.energy_ratios(ed, sd, lengths=lengths, return_alpha=True, **{third: td})
    assert torch.equal(again, ratios) and torch.equal(again_a, alpha)


def test_packets_over_more_than_eight_chunks():
    """the row of 17 C + 3 samples (18 chunks) whole and in packets cut at 8 C, at 1 and at (9 C + 5, 16 C): a packet's
    partials are added on top of what the accumulator holds, through the unrolled body and the remainder"""
    ops = _ops()
    L = 17 * C + 3
    e, s, n, want, _ = _draw(L, 4)
    ed, sd, nd = _gpu(e, s, n)

    def run(cuts):
        acc = ops.score_state(1, DEV)
        edges = [0] + list(cuts) + [L]
        for a, b in zip(edges[:-1], edges[1:]):
            assert ops.score_accumulate(acc, ed[a:b], sd[a:b], noise=nd[a:b]) is acc
        return ops.score_finalize(acc, "noise"), acc.clone()
    for name, cuts in {"single": (), "8C | rest": (8 * C,), "1 | rest": (1,), "9C+5 | 16C | rest": (9 * C + 5, 16 * C)}.items():
        first = run(cuts)
        _close("packets %s" % name, first[0][0].cpu().numpy(), want)
        again = run(cuts)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]), name


def test_seventy_rows():
    """B = 70, lengths 2 + 37 b mod 299: the second workgroup of the finalize and rows behind 64 everywhere.  Rows 64 and
    69 are the exact dyadic one-sample row ((inf, 0, 0), alphas [0.5, -2.0]), row 66 is empty (all NaN); every other row
    against float64.  Then the same through a caller-owned accumulator, twice: x + x is exact, so the accumulator doubles
    bit for bit and the second pass read what the first had left at every row."""
    ops = _ops()
    B = 70
    lengths = [2 + (37 * b) % 299 for b in range(B)]
    dyadic = (np.float32([0.25]), np.float32([0.5]), np.float32([-0.125]))
    rows = [_draw(L, b % 9)[:3] for b, L in enumerate(lengths)]
    for b in (64, 69):
        rows[b], lengths[b] = dyadic, 1
    rows[66], lengths[66] = None, 0
    P = 300 + 5
    ed, sd, nd = _ragged(rows, P)
    ratios_d, alpha_d = ops.energy_ratios(ed, sd, noise=nd, lengths=lengths, return_alpha=True)
    ratios, alpha = ratios_d.cpu().numpy(), alpha_d.cpu().numpy()
    assert ratios.shape == (B, 3) and alpha.shape == (B, 2)
    worst = 0.0
    for b in range(B):
        if b in (64, 69):
            assert ratios[b].tolist() == [np.inf, 0.0, 0.0] == list(score_ref.energy_ratios(*dyadic)), (b, ratios[b])
            assert alpha[b].tolist() == [0.5, -2.0] == list(score_ref.alphas(*dyadic)), (b, alpha[b])
        elif b == 66:
            assert np.isnan(ratios[b]).all() and np.isnan(alpha[b]).all()
        else:
            want, want_a = np.array(score_ref.energy_ratios(*rows[b])), np.array(score_ref.alphas(*rows[b]))
            assert np.isfinite(ratios[b]).all() and np.isfinite(want).all(), b
            d = np.abs(ratios[b] - want).max()
            worst = max(worst, d)
            assert d <= TOL_DB, (b, lengths[b], ratios[b], want)
            assert (np.abs(alpha[b] - want_a) <= TOL_ALPHA * np.abs(want_a)).all(), (b, alpha[b], want_a)
    print("70 rows: worst |d| %.3g dB; rows 63 .. 69 %s" % (worst, ratios[63:]))
    acc = ops.score_state(B, DEV)
    assert ops.score_accumulate(acc, ed, sd, noise=nd, lengths=lengths) is acc
    once = acc.clone()
    got, got_a = ops.score_finalize(acc, "noise", return_alpha=True)
    same = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))      # noqa: E731  (bits: NaN rows included)
    assert same(got, ratios_d) and same(got_a, alpha_d)
    assert not once[66].any() and bool((once[:, 0] > 0)[[b for b in range(B) if b != 66]].all())
    ops.score_accumulate(acc, ed, sd, noise=nd, lengths=lengths)
    assert torch.equal(acc, once + once)


def _f1_rows(hard, target, lengths):
    from packages.models.utils import f1_loss
    rows = []
    for b, n in enumerate(lengths):
        rows.append(torch.stack(list(f1_loss(hard[b, :n].reshape(-1).long(), target[b, :n].reshape(-1).long()))))
    return torch.stack(rows)


# (5, 24, 512): 12 288 values (three full chunks of 4096), 4096 (one chunk exactly, the next exits), 4608, 0 and 8704 -- rows
# of several chunks next to chunks that exit at once; (70, 9, 7): rows behind 64
@pytest.mark.parametrize("shape,lengths", [((3, 7, 1), [7, 1, 0]), ((3, 5, 513), [5, 1, 0]), ((1, 370, 513), [370]),
                                           ((5, 24, 512), [24, 8, 9, 0, 17]), ((70, 9, 7), [[9, 4, 0, 1, 7][b % 5] for b in range(70)])])
def test_confusion_counts(shape, lengths):
    ops = _ops()
    B, T, Y = shape
    rng = np.random.default_rng(B * T * Y)
    hard = (rng.random(shape) > 0.45).astype(np.float32)
    target = (rng.random(shape) > 0.6).astype(np.float32)
    logit = (rng.uniform(0.01, 3.0, shape) * np.where(rng.random(shape) > 0.5, 1.0, -1.0)).astype(np.float32)
    hard_of_logit = (torch.sigmoid(T_(logit)) > 0.5).numpy()
    want, want_l = score_ref.confusion(hard, target, lengths), score_ref.confusion(hard_of_logit, target, lengths)
    assert want.sum(axis=1).tolist() == [n * Y for n in lengths]
    for arr in (hard, target, logit):                       # behind the lengths: NaN, which no count may see
        for b, n in enumerate(lengths):
            arr[b, n:] = NAN
    hd, td, ld = _gpu(hard, target, logit)
    counts = ops.confusion_counts(hd, td, lengths)
    assert counts.dtype == torch.int64 and counts.shape == (B, 4) and counts.is_cuda
    assert np.array_equal(counts.cpu().numpy(), want)
    f1 = ops.f1_from_counts(counts)
    assert f1.dtype == torch.float32 and torch.equal(f1.cpu(), _f1_rows(T_(hard), T_(target), lengths))
    by_logit = ops.confusion_counts(ld, td, torch.LongTensor(lengths), logits=True)
    assert np.array_equal(by_logit.cpu().numpy(), want_l)
    assert torch.equal(ops.f1_from_counts(by_logit).cpu(), _f1_rows(T_(hard_of_logit.astype(np.float32)), T_(target), lengths))
    assert ops.confusion_counts(hd, td, lengths, counts=counts) is counts
    assert np.array_equal(counts.cpu().numpy(), 2 * want)
    if lengths == [T] * B:                                   # no lengths: every frame counts
        assert np.array_equal(ops.confusion_counts(hd, td).cpu().numpy(), want)
    if Y == 1:                                               # (B, T) is (B, T, 1)
        assert np.array_equal(ops.confusion_counts(hd[..., 0], td[..., 0], lengths).cpu().numpy(), want)


def test_dropin_metrics_take_numpy_and_tensors():
    from packages import metrics
    e, s, n, want, alpha = _draw(C + 1, 9)
    got = metrics.energy_ratios(e, s, n)
    assert all(isinstance(v, float) for v in got)
    _close("packages.metrics.energy_ratios (numpy)", got, want)
    planes = metrics.si_sdr_components(e, s, n)
    for name, a, b in zip(("s_target", "e_noise", "e_art"), planes, score_ref.components(e, s, n)):
        assert isinstance(a, np.ndarray) and a.shape == e.shape
        assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max(), name          # float32 planes of float32 input
    ed, sd, nd = _gpu(e, s, n)
    got_t = metrics.energy_ratios(ed, sd, nd)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float64 for v in got_t)
    _close("packages.metrics.energy_ratios (tensors)", [float(v) for v in got_t], want)
    planes_t = metrics.si_sdr_components(ed, sd, nd)
    assert all(isinstance(p, torch.Tensor) and p.is_cuda and p.shape == ed.shape for p in planes_t)
    assert torch.allclose(sum(planes_t), ed, rtol=0, atol=1e-6)


def _wav_pairs(tmp_path):
    from scipy.io import wavfile
    rng = np.random.default_rng(99)
    pairs = []
    for i in range(2):
        t = np.arange(6000) / 16000.0
        clean = 0.3 * np.sin(2 * np.pi * (180 + 70 * i) * t) * (1 + np.sin(2 * np.pi * 3 * t)) + 0.02 * rng.standard_normal(6000)
        clean[:1500] *= 0.01                                 # a quiet lead-in: both VAD classes occur
        noisy = clean + 0.1 * rng.standard_normal(6000)
        pc, pn = str(tmp_path / ("clean%d.wav" % i)), str(tmp_path / ("noisy%d.wav" % i))
        wavfile.write(pc, 16000, np.round(clean * 20000).astype(np.int16))
        wavfile.write(pn, 16000, np.round(noisy * 20000).astype(np.int16))
        pairs.append((pn, pc))
    return pairs


def test_evaluator_scores_on_the_gpu(tmp_path):
    from scipy.io import wavfile
    from avvad import train as TR
    from packages.models.Audio_Net import DeepVAD_audio
    ops = _ops()
    pairs = _wav_pairs(tmp_path)
    make = lambda: DeepVAD_audio(1, 16, 513)                 # noqa: E731
    kw = dict(wav_list=[p[0] for p in pairs], clean_of=dict(pairs))
    out, wav, sc = (str(tmp_path / d) for d in ("out", "wav", "scores"))
    TR.evaluate_main("audio", make, out_dir=out, resynth_dir=wav, score_dir=sc, **kw)
    assert sorted(os.listdir(sc)) == ["noisy0_scores.pt", "noisy1_scores.pt"]
    for i, (pn, pc) in enumerate(pairs):
        d = torch.load(os.path.join(sc, "noisy%d_scores.pt" % i), weights_only=True)
        assert set(d) == {"tp", "tn", "fp", "fn"} | set(TR.SCORE_KEYS)
        assert all(isinstance(d[k], int) for k in ("tp", "tn", "fp", "fn")) and all(isinstance(d[k], float) for k in TR.SCORE_KEYS)
        label = torch.load(os.path.join(out, "noisy%d_label.pt" % i), weights_only=True)
        hard = torch.load(os.path.join(out, "noisy%d_y_hat_hard.pt" % i), weights_only=True)
        assert d["tp"] + d["tn"] + d["fp"] + d["fn"] == label.numel() == hard.numel() > 0
        assert d["tp"] + d["fp"] == int(hard.sum()) and d["tp"] + d["fn"] == int(label.sum())
        fs, enhanced = wavfile.read(os.path.join(wav, "noisy%d_enhanced.wav" % i))
        noisy, clean = TR.load_waveform(pn)[0], TR.load_waveform(pc)[0]
        assert enhanced.dtype == np.float32 and enhanced.shape == (6000,) == tuple(clean.shape)
        ed, cd, xd = T_(enhanced).to(DEV), clean.to(DEV), noisy.to(DEV)
        want = ops.energy_ratios(ed, cd, mixture=xd)[0].tolist() + [float(ops.energy_ratios(xd, cd, mixture=xd)[0, 0])]
        _close("utterance %d" % i, [d[k] for k in TR.SCORE_KEYS], want)
        ref = list(score_ref.energy_ratios(enhanced, clean.numpy(), noisy.numpy().astype(np.float64) - clean.numpy()))
        ref.append(score_ref.energy_ratios(noisy.numpy(), clean.numpy())[0])
        print("utterance %d: scores %s, float64 reference %s" % (i, [d[k] for k in TR.SCORE_KEYS], ref))
        assert np.abs(np.array([d[k] for k in TR.SCORE_KEYS]) - np.array(ref)).max() <= TOL_DB       # (all below 60 dB)
        assert max(ref) <= 60.0
        assert TR.score_utt(ed, cd, xd) == {k: d[k] for k in TR.SCORE_KEYS}
    tables = TR.metrics_main(out, score_dir=sc)
    assert set(tables) == {"classifier", "enhancement"}
    assert list(tables["enhancement"]["all"]) == list(TR.SCORE_KEYS) == ["si_sdr", "si_sir", "si_sar", "input_si_sdr"]
    assert list(tables["classifier"]["all"]) == ["accuracy", "precision", "recall", "f1score"]
    # without score_dir: the files of before, and nothing more
    out0, wav0 = str(tmp_path / "out0"), str(tmp_path / "wav0")
    TR.evaluate_main("audio", make, out_dir=out0, resynth_dir=wav0, **kw)
    assert sorted(os.listdir(out0)) == sorted(os.listdir(out)) and sorted(os.listdir(wav0)) == sorted(os.listdir(wav))
    assert len(os.listdir(out0)) == 6 and sorted(os.listdir(tmp_path)) == sorted(
        ["clean0.wav", "clean1.wav", "noisy0.wav", "noisy1.wav", "out", "wav", "scores", "out0", "wav0"])
    for f in os.listdir(out0):
        assert torch.equal(torch.load(os.path.join(out0, f), weights_only=True), torch.load(os.path.join(out, f), weights_only=True))
    assert list(TR.metrics_main(out0)["all"]) == ["accuracy", "precision", "recall", "f1score"]
    with pytest.raises(ValueError, match="clean_of"):
        TR.evaluate_main("audio", make, out_dir=out0, wav_list=kw["wav_list"], score_dir=sc)
