"""CPU tests of the scores (csrc/scores.hip): the float64 reference tests/score_ref.py against what the reference's own
``energy_ratios`` / ``si_sdr_components`` / ``f1_loss`` produced (tests/golden/scores.npz), and the check the GPU tests'
tolerance rests on -- the closed form in six chunk-summed inner products against the planes-and-norms form, to 1e-6 dB
over lengths 255 .. 70 001, artefact levels -5 .. 80 dB and noise gains 1 .. 1e-3.  Host-side pieces that need no GPU:
``f1_from_counts``, the chunk constant and the workspace query, the refusals of the C ABI.  And the twins of the GPU
tests past 8 chunks and 64 rows: the five rows of 8 to 17 chunks draw on their first seed, and cutting any of them to the
chunks a finish would keep if it stopped after (or skipped) the unrolled body of its sum moves every ratio of the float64
reference by over 100 tolerances; the confusion shapes hold the value counts their names promise."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import score_ref
from conftest import ROOT, load_golden

TOL_DB = 1e-6


@pytest.fixture(scope="module")
def golden():
    return load_golden("scores")


@pytest.mark.parametrize("k", range(4))
def test_reference_matches_the_recorded_outputs(golden, k):
    e, s, n = (golden["c%d_%s" % (k, name)] for name in ("s_hat", "s", "n"))
    assert e.dtype == np.float32 and e.size <= 1500
    want = golden["c%d_ratios" % k]
    got = np.array(score_ref.energy_ratios(e, s, n))
    print("case %d (L = %d): ratios %s, |d| %s dB" % (k, e.size, want, np.abs(got - want)))
    assert np.all(np.isfinite(want)) and np.all(np.abs(got - want) <= 1e-9)
    for name, a, b in zip(("s_target", "e_noise", "e_art"), score_ref.components(e, s, n), golden["c%d_components" % k]):
        assert np.allclose(a, b, rtol=1e-12, atol=1e-15), name
    assert abs(score_ref.energy_ratios(e, s)[0] - want[0]) <= 1e-9 and np.isnan(score_ref.energy_ratios(e, s)[1:]).all()


@pytest.mark.parametrize("k", range(2))
def test_counts_give_the_recorded_f1(golden, k):
    from avvad import ops
    pred, target, lengths = golden["g%d_pred" % k], golden["g%d_target" % k], golden["g%d_lengths" % k]
    counts = score_ref.confusion(pred, target, lengths)
    assert counts.sum(axis=1).tolist() == [int(n) * pred.shape[2] for n in lengths]
    got = ops.f1_from_counts(torch.from_numpy(counts))
    assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(golden["g%d_f1" % k]))


@pytest.mark.parametrize("L", [255, 256, 4097, 16387, 70001])
def test_gram_form_matches_the_planes_form(L):
    worst = 0.0
    for j, art_db in enumerate((-5.0, 20.0, 40.0, 80.0)):
        for i, g in enumerate((1.0, 0.1, 1e-3)):
            e, s, n = score_ref.mix(np.random.default_rng(1000 * L + 10 * j + i), L, g, art_db)
            want = np.array(score_ref.energy_ratios(e, s, n))
            got = np.array(score_ref.gram_ratios(e, s, n, chunk=4096))
            d = np.abs(got - want).max()
            worst = max(worst, d)
            assert np.isfinite(want).all() and d <= TOL_DB, (L, art_db, g, want, got)
    print("L = %d: worst |gram - planes| = %.3g dB" % (L, worst))


def test_gram_form_edge_values():
    z = np.zeros(0, dtype=np.float32)
    assert np.isnan(score_ref.gram_ratios(z, z, z)).all() and np.isnan(score_ref.energy_ratios(z, z, z)).all()
    s = np.array([1.0, -2.0, 0.5], dtype=np.float32)
    n = np.array([2.0, 1.0, 0.0], dtype=np.float32)          # orthogonal to s
    want, got = score_ref.energy_ratios(2 * s, s, n), score_ref.gram_ratios(2 * s, s, n)
    assert want[0] == got[0] == np.inf and np.isnan(got[1]) == np.isnan(want[1])


def test_chunk_constant_and_workspace_query():
    from avvad import _lib as L, ops
    h = L.lib()
    header = open(os.path.join(ROOT, "include", "avvad.h")).read()
    chunk = int(re.search(r"#define AVVAD_SCORE_CHUNK (\d+)", header).group(1))
    assert chunk == L.SCORE_CHUNK == ops.SCORE_CHUNK
    # one 6-double partial per (row, chunk), rounded up to 256 bytes: five chunks fit 256 bytes, the sixth does not
    assert h.avvad_score_workspace(1, 1) == h.avvad_score_workspace(1, 5 * chunk) == 256
    assert h.avvad_score_workspace(1, 5 * chunk + 1) == 512
    assert h.avvad_score_workspace(16, 80000) == 16 * -(-80000 // chunk) * 48
    assert h.avvad_score_workspace(0, 100) == h.avvad_score_workspace(1, 0) == h.avvad_score_workspace(65536, 1) == 0


def test_refusals_need_no_gpu():
    from avvad import _lib as L, ops
    h = L.lib()
    p = lambda v: C.c_void_p(v)                              # noqa: E731  (never dereferenced: every call is refused first)
    ok = (p(4096), 10, p(8192), 10, None, 0, 0, None, p(16384), 1, 10, p(65536), 256, None)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return h.avvad_score_accumulate(*a)
    assert call(a0=None) == call(a2=None) == call(a8=None) == call(a11=None) == -1
    assert call(a1=9) == call(a3=9) == -1                    # a pitch below L
    assert call(a6=1) == call(a6=3) == call(a4=p(4096)) == -1    # the third signal and its mode go together
    assert call(a4=p(4096), a5=9, a6=2) == -1
    assert call(a8=p(16388)) == call(a11=p(65540)) == call(a11=p(65536 + 16)) == -1
    assert call(a9=0) == call(a10=0) == -1
    assert call(a12=255) == -2
    assert h.avvad_score_finalize(None, 1, 0, p(4096), None, None) == -1
    assert h.avvad_score_finalize(p(4096), 1, 3, p(8192), None, None) == h.avvad_score_finalize(p(4096), 0, 0, p(8192), None, None) == -1
    assert h.avvad_score_finalize(p(4096), 1, 0, p(8196), None, None) == h.avvad_score_finalize(p(4096), 1, 0, p(8192), p(4), None) == -1
    assert h.avvad_confusion_accumulate(p(4096), 0, p(8192), None, p(16388), 1, 2, 3, None) == -1
    assert h.avvad_confusion_accumulate(p(4096), 2, p(8192), None, p(16384), 1, 2, 3, None) == -1
    assert h.avvad_confusion_accumulate(None, 0, p(8192), None, p(16384), 1, 2, 3, None) == -1
    assert h.avvad_confusion_accumulate(p(4096), 0, p(8192), None, p(16384), 1, 0, 3, None) == -1
    with pytest.raises(L.AvvadError, match="GPU"):
        ops.energy_ratios(torch.zeros(4), torch.zeros(4))
    with pytest.raises(L.AvvadError, match="GPU"):
        ops.score_state(1, "cpu")
    with pytest.raises(L.AvvadError, match="GPU"):
        ops.confusion_counts(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3))


def _chunk():
    from avvad import _lib as L
    return L.SCORE_CHUNK


def test_many_chunk_rows_draw_at_once_and_a_truncated_sum_cannot_pass():
    """The GPU test's five rows (8, 8 + 1 sample, 9, 16, 17 chunks), noise and mixture as the third signal: every
    reference ratio in [-10, 60] dB on the first seed; on the float64 reference alone, a row longer than 8 chunks cut to
    its first 8 chunks, and the 8-chunk row cut to 7, moves each of its three ratios by more than 100 * TOL_DB -- so a
    finish that stops after the unrolled body of its sum, or skips it, is far outside the tolerance."""
    Cn = _chunk()
    lengths = score_ref.many_chunk_lengths(Cn)
    assert lengths == [8 * Cn, 8 * Cn + 1, 9 * Cn + 5, 16 * Cn, 17 * Cn + 3]
    assert [-(-n // Cn) for n in lengths] == [8, 9, 10, 16, 18] and [n // Cn % 8 for n in lengths] == [0, 0, 1, 0, 1]
    smallest = np.inf
    for k, n_ in enumerate(lengths):
        e, s, n, want, _ = score_ref.draw(n_, k)
        assert score_ref.draw_misses(n_, k) == 0 and np.all((want >= -10.0) & (want <= 60.0)), (k, want)
        x, n_mix = score_ref.mixture_of(s, n)
        want_mix = np.array(score_ref.energy_ratios(e, s, n_mix))
        assert np.all((want_mix >= -10.0) & (want_mix <= 60.0)), (k, want_mix)
        cut = 7 * Cn if n_ == 8 * Cn else 8 * Cn
        for third, full in ((n, want), (n_mix, want_mix)):
            moved = np.abs(np.array(score_ref.energy_ratios(e[:cut], s[:cut], third[:cut])) - full)
            print("row of %d samples cut to %d: ratios move by %s dB" % (n_, cut, moved))
            assert moved.min() > 100 * TOL_DB, (n_, cut, moved)
            smallest = min(smallest, moved.min())
    print("smallest move %.3g dB" % smallest)


def test_many_row_lengths_and_confusion_shapes_are_what_the_gpu_tests_name():
    lengths = [2 + (37 * b) % 299 for b in range(70)]
    assert min(lengths) == 2 and max(lengths) <= 300 and len(set(lengths)) == 70
    source = open(os.path.join(ROOT, "audio-visual-vad_amd", "csrc", "scores.hip")).read()
    conf = int(re.search(r"constexpr int CONF_CHUNK = (\d+);", source).group(1))
    assert conf == 4096
    values = [n * 512 for n in (24, 8, 9, 0, 17)]
    assert values == [3 * conf, conf, conf + 512, 0, 2 * conf + 512] == [12288, 4096, 4608, 0, 8704]
    assert -(-24 * 512 // conf) == 3                          # the grid: three chunks per row, so row 1's second chunk exits
