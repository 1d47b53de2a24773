"""CPU side of the STOI / ESTOI cases past one loop trip (stoi_ref.LONG_CASE_NAMES; the GPU side is
tests/test_stoi_long_gpu.py): more than 256 frames (invert_kept's second workgroup), more than 1024 (the second trip of
keep_frames' maximum and of its compaction scan, whose list position is carried from trip to trip), frames dropped on both
sides of frame 1024, and one row whose loudest frame lies behind frame 1024.

Here, on the float64 reference alone, so that no GPU test can hide behind them: the conditions the inputs must meet (with
the case table printed); the float32 stand-in's worst error over the long cases -- the score within the constant measured
over the short ones, the gradient within a constant of its own, which two 16 kHz rows need; the hand-written chain against
autograd in float64; and the mutants -- each restates one way a kernel goes wrong past a trip, and each must be rejected by
the very functions the GPU tests call (stoi_ref.check_info / check_d, stoi_loss_ref.check_gradient)."""
import numpy as np
import pytest

import stoi_loss_ref as G
import stoi_ref as R

LONG = R.LONG_CASE_NAMES
NOISY = "k10_166700_noisy"                    # the one long case whose STOI gradient is not compared
MID = "k10_60000_mid"                         # between 256 and 1024 frames
PAST_A_TRIP = [n for n in LONG if n != MID]


def _mask(name):
    fs, x, _ = R.case(name)
    x = np.asarray(x, dtype=np.float64)
    return R.keep_mask(R.resample(x) if fs == 16000 else x)


def test_the_long_cases_meet_their_conditions():
    both_sides = []
    print()
    for name in LONG:
        r, m, (gap, clipped, total), mask = R.reference(name), R.case_margin(name), G.case_clip(name), _mask(name)
        lo, hi = int((~mask[:R.KEEP_TRIP]).sum()), int((~mask[R.KEEP_TRIP:]).sum())
        print("%-24s fs %5d n %6d frames %4d kept %4d (dropped %3d before frame 1024, %3d behind) margin %.3f dB clip gap %.2e "
              "clipped %5d of %d" % (name, R.case(name)[0], R.case(name)[1].size, r["frames"], r["kept"], lo, hi, m, gap, clipped, total))
        assert m >= R.MIN_MARGIN_DB, name
        assert r["M"] == r["kept"] - 1 and r["segments"] == r["M"] - 29
        if r["frames"] > R.KEEP_TRIP and r["kept"] > R.KEEP_TRIP and lo > 0 and hi > 0:
            both_sides.append(name)
    assert len(both_sides) >= 2 and {R.case(n)[0] for n in both_sides} == {10000, 16000}, both_sides
    assert all(R.reference(n)["frames"] > R.KEEP_TRIP for n in PAST_A_TRIP)
    # the STOI gradient of every long case but one is compared, and every compared case has clipped elements
    assert G.grad_cases(2, LONG) == list(LONG)
    assert G.grad_cases(1, LONG) == [n for n in LONG if n != NOISY] and G.case_clip(NOISY)[0] < G.MIN_CLIP_GAP
    assert all(G.case_clip(n)[1] > 0 for n in G.grad_cases(1, LONG))
    # invert_kept's second workgroup with all 16 waves of keep_frames loaded: kept frames at and behind frame 256
    mid, mask = R.reference(MID), _mask(MID)
    assert G.INVERT_BLOCK < mid["frames"] <= R.KEEP_TRIP and mask[G.INVERT_BLOCK:].sum() > 30 and (~mask[G.INVERT_BLOCK:]).sum() > 0
    # the short cases keep their samples: the tables are separate
    assert not set(LONG) & set(R.CASE_NAMES) and "committed" in R.CASE_NAMES and len(R.CASE_NAMES) == 15


def test_the_loudest_frame_case_needs_the_whole_rows_maximum():
    """its loudest frame lies in the second trip, and the kept set changes if the maximum is taken from the first alone; both
    the true and the wrong threshold keep the margin, so either decision is the same in float32"""
    fs, x, _ = R.case(R.LOUD_TAIL_CASE)
    e = R.energies(np.asarray(x, dtype=np.float64))
    top, first = float(np.max(e)), float(np.max(e[:R.KEEP_TRIP]))
    true, wrong = (top - R.DYN_RANGE - e) < 0, (first - R.DYN_RANGE - e) < 0
    print("loudest frame %d of %d: %.2f dB over the first %d frames' loudest; kept %d, with the first trip's maximum %d; margins "
          "%.3f and %.3f dB" % (int(np.argmax(e)), e.size, top - first, R.KEEP_TRIP, true.sum(), wrong.sum(),
                                np.abs(e - (top - R.DYN_RANGE)).min(), np.abs(e - (first - R.DYN_RANGE)).min()))
    assert int(np.argmax(e)) >= R.KEEP_TRIP and top - first > 3.0
    assert np.array_equal(true, _mask(R.LOUD_TAIL_CASE)) and true.sum() == R.reference(R.LOUD_TAIL_CASE)["kept"]
    assert wrong.sum() >= true.sum() + 8 and not (true & ~wrong).any()          # the blocks: kept by the wrong rule alone
    assert (wrong & ~true)[:R.KEEP_TRIP].sum() >= 8
    assert np.abs(e - (first - R.DYN_RANGE)).min() >= R.MIN_MARGIN_DB and R.case_margin(R.LOUD_TAIL_CASE) >= R.MIN_MARGIN_DB


def test_standin_over_the_long_cases():
    """the float32 stand-in against float64 over the long cases.  The score stays within MEASURED_STANDIN, the figure of the
    short cases, so GPU_BOUND holds unchanged.  The gradient of the two long 16 kHz rows does not stay within
    MEASURED_STANDIN_GRAD (2.9e-6): the long cases have MEASURED_STANDIN_GRAD_LONG, this test's worst figure rounded up, and
    the GPU gets 8 times that."""
    worst_d = worst_g = 0.0
    print()
    for name in LONG:
        fs, x, y = R.case(name)
        ref, got = R.reference(name), R.score(x, y, fs, f32=True)
        assert (ref["frames"], ref["kept"], ref["segments"]) == (got["frames"], got["kept"], got["segments"]), name
        e = max(abs(ref["stoi"] - got["stoi"]), abs(ref["estoi"] - got["estoi"]))
        worst_d = max(worst_d, e)
        line = "%-24s |stand-in - float64| = %.3g;" % (name, e)
        for which in (1, 2):
            if name not in G.grad_cases(which, (name,)):
                line += "  STOI gradient not compared;"
                continue
            eg = G.err(G.manual_grad(x, y, fs, which, f32=True), G.reference(name, which)[1])
            worst_g = max(worst_g, eg)
            line += "  %s gradient %.3g;" % ("STOI" if which == 1 else "ESTOI", eg)
        print(line)
    print("worst score %.3g (stand-in bound %.3g, GPU bound %.3g), worst gradient %.3g (stand-in bound %.3g, GPU bound %.3g)"
          % (worst_d, R.MEASURED_STANDIN, R.GPU_BOUND, worst_g, G.MEASURED_STANDIN_GRAD_LONG, G.GPU_GRAD_BOUND_LONG))
    assert 0.0 < worst_d <= R.MEASURED_STANDIN
    assert G.GPU_GRAD_BOUND_LONG == 8 * G.MEASURED_STANDIN_GRAD_LONG and all(G.grad_bound(n) == G.GPU_GRAD_BOUND_LONG for n in LONG)
    assert all(G.grad_bound(n) == G.GPU_GRAD_BOUND for n in R.CASE_NAMES)
    assert 0.5 * G.MEASURED_STANDIN_GRAD_LONG <= worst_g <= G.MEASURED_STANDIN_GRAD_LONG


@pytest.mark.parametrize("name", LONG)
def test_hand_written_chain_is_the_autograd_gradient(name):
    fs, x, y = R.case(name)
    for which in (1, 2):
        g = G.manual_grad(x, y, fs, which)
        e = G.err(g, G.reference(name, which)[1])
        print("%-24s which %d: closed forms against autograd %.2g" % (name, which, e))
        assert e <= 1e-12
        assert G.check_gradient(name, which, g) in (None, e)     # and the check passes what is right


def _rejected(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def _mutant_result(name, mutant):
    fs, x, y = R.case(name)
    got = R.score(x, y, fs, **R.LONG_MUTANTS[mutant])
    return [got["stoi"], got["estoi"]], [got["frames"], got["kept"], got["segments"]]


def test_the_checks_pass_the_reference_itself():
    for name in LONG:
        ref = R.reference(name)
        R.check_scores(name, [ref["stoi"], ref["estoi"]], [ref["frames"], ref["kept"], ref["segments"]])


def test_max_of_first_trip_is_rejected_by_the_kept_count():
    d, info = _mutant_result(R.LOUD_TAIL_CASE, "max_of_first_trip")
    ref = R.reference(R.LOUD_TAIL_CASE)
    print("max_of_first_trip on %s: kept %d for %d, score moved by %.3g" % (R.LOUD_TAIL_CASE, info[1], ref["kept"], R.score_error(R.LOUD_TAIL_CASE, d)))
    assert info[0] == ref["frames"] and info[1] > ref["kept"]
    _rejected(R.check_info, R.LOUD_TAIL_CASE, info)
    _rejected(R.check_scores, R.LOUD_TAIL_CASE, d, info)
    # a row without a frame near either threshold cannot tell: which is why the case above exists
    d, info = _mutant_result("k10_211650_both_sides", "max_of_first_trip")
    R.check_scores("k10_211650_both_sides", d, info)


@pytest.mark.parametrize("mutant", ["frames_of_one_trip", "scan_not_carried"])
def test_a_lost_trip_is_rejected_by_info_and_by_the_score(mutant):
    for name in PAST_A_TRIP:
        d, info = _mutant_result(name, mutant)
        print("%s on %-24s info %s for %s, score moved by %.3g (GPU bound %.3g)"
              % (mutant, name, info, [R.reference(name)[k] for k in ("frames", "kept", "segments")], R.score_error(name, d), R.GPU_BOUND))
        _rejected(R.check_info, name, info)
        _rejected(R.check_d, name, d)
    d, info = _mutant_result(MID, mutant)                    # within one trip nothing is lost
    R.check_scores(MID, d, info)


@pytest.mark.parametrize("name", LONG)
def test_positions_of_one_block_is_rejected_by_the_gradient_bound(name):
    fs, x, y = R.case(name)
    for which in (1, 2):
        if name not in G.grad_cases(which, (name,)):
            continue
        g = G.manual_grad(x, y, fs, which, mutant="positions_of_one_block")
        print("positions_of_one_block on %-24s which %d: gradient error %.3g (GPU bound %.3g)"
              % (name, which, G.err(g, G.reference(name, which)[1]), G.grad_bound(name)))
        _rejected(G.check_gradient, name, which, g)


def test_positions_of_one_block_passes_within_256_frames():
    """which is why the short cases cannot tell"""
    fs, x, y = R.case("k10_9001_half")
    assert G.check_gradient("k10_9001_half", 2, G.manual_grad(x, y, fs, 2, mutant="positions_of_one_block")) <= 1e-12
