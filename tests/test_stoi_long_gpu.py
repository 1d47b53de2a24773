"""GPU tests of STOI / ESTOI and their training loss (csrc/stoi.hip, ops.stoi, ops.stoi_loss) past one loop trip: the cases
stoi_ref.LONG_CASE_NAMES of 467 to 1683 frames and a batch of 70 rows, where the other two files stop at 233 frames and 5 rows.

What runs here for the first time: the second trip of keep_frames' maximum and of its compaction scan (more than 1024
frames; the list position is carried from trip to trip, and one case has its loudest frame in the second trip),
invert_kept's second workgroup (more than 256 frames), the second workgroup of finalize and the second trip of loss_sum
(more than 64 rows), the engine products at 2 B mf = 13 456 rows and the segment passes at up to 1330 segments per row.

The checks are the other two files' own -- info exactly, |d - float64| <= stoi_ref.GPU_BOUND, the gradient's error within
stoi_loss_ref.grad_bound (8 x the float32 stand-in's worst figure over the long cases), d of the loss = ops.stoi's bits, a
row in a batch = the row alone, bit for bit -- and tests/test_stoi_long_cpu.py shows on the CPU that a kernel that stops
after a trip, restarts its list, takes the maximum from the first trip or answers -1 behind frame 256 fails them.  Every
figure is printed."""
import numpy as np
import pytest
import torch

import stoi_loss_ref as G
import stoi_ref as R
import test_stoi_gpu as SG
import test_stoi_loss_gpu as LG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LONG = R.LONG_CASE_NAMES
PER_RATE = ["k10_211650_both_sides", "k16_345004_both_sides"]
CYCLE_10K = ["k10_4097_one_segment", "k10_4096_no_segment", "k10_6000_light", "k10_6000_heavy", "k10_9001_half", "short"]


def _ops():
    from avvad import ops
    return ops


def _i64(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("name", LONG)
def test_scores_and_info_against_float64(name):
    d, info = SG._alone(name)
    SG._check(name, d, info)
    assert R.reference(name)["frames"] > G.INVERT_BLOCK and R.reference(name)["segments"] > 300


@pytest.mark.parametrize("name", PER_RATE)
def test_both_equals_the_single_calls_and_runs_repeat(name):
    assert R.reference(name)["kept"] > R.KEEP_TRIP
    SG.test_both_equals_the_single_calls_and_runs_repeat(name)


@pytest.mark.parametrize("name", LONG)
def test_value_and_gradient_against_float64(name):
    """d has ops.stoi's bits, loss = float32(-d), the gradient is finite and within its bound of float64's (the STOI
    gradient of the -5 dB case prints why it is not compared)"""
    LG.test_value_and_gradient_against_float64(name)


@pytest.mark.parametrize("fs, names", [
    (10000, ["k10_211650_both_sides", "k10_4097_one_segment", "short", "k10_9001_half"]),
    (16000, ["k16_345004_both_sides", "k16_8705", "short", "k16_9731"]),
])
def test_ragged_batch_with_a_long_row_keeps_every_rows_bits(fs, names, lib_options):
    """B = 4 whose frame counts differ 20-fold and more inside one plan (1652 / 1683 frames beside 31 / 41, a row with frames
    and no segment, a row shorter than a frame), NaN behind every length, a pitch wider than L: every row's d and gradient
    have the bits they have alone, at max_cus 0 and 24; exact zeros behind each length; the run repeats bit for bit"""
    ops = _ops()
    L = max(R.case(n)[1].size for n in names if n != "short")
    P = L + 37
    x, y, lengths = LG._batch(names, P)
    assert R.reference(names[0])["frames"] >= 20 * R.reference(names[1])["frames"] > 0
    for which in (1, 2):
        runs = []
        for cap in (0, 24, 0):
            lib_options("max_cus", cap)
            wide = y.clone().requires_grad_(True)
            loss, d = ops.stoi_loss(wide[:, :L], x[:, :L], lengths=lengths, fs=fs, extended=which == 2, return_scores=True)
            loss.backward()
            g = wide.grad
            assert d.shape == (4,) and g.shape == (4, P) and bool(torch.isfinite(g).all())
            total = 0.0
            for b, n in enumerate(names):
                assert torch.count_nonzero(g[b, lengths[b]:]).item() == 0
                total += float(d[b])
                if n == "short":
                    assert float(d[b]) == 1e-5 and torch.count_nonzero(g[b]).item() == 0
                    continue
                _, da, ga = LG._alone(n, which)
                assert torch.equal(_i64(d[b:b + 1]), _i64(da)), (n, cap)
                assert torch.equal(g[b, :lengths[b]], ga), (n, cap)
            assert float(loss.detach()) == float(np.float32(-total))
            runs.append((loss.detach(), g.clone()))
        assert torch.equal(runs[0][0], runs[2][0]) and torch.equal(runs[0][1], runs[2][1])
    for cap in (0, 24):                                      # the score's own entry point on the same batch
        lib_options("max_cus", cap)
        d, info = ops.stoi(x[:, :L], y[:, :L], lengths=lengths, fs=fs, both=True, return_info=True)
        for b, n in enumerate(names):
            if n == "short":
                assert info[b].tolist() == [0, 0, 0] and d[b].tolist() == [1e-5, 1e-5]
                continue
            da, ia = SG._alone(n)
            assert torch.equal(_i64(d[b]), _i64(da)) and torch.equal(info[b], ia), (n, cap)


def test_more_than_64_rows():
    """B = 70 at 10 kHz, L = 9001: finalize's second workgroup and loss_sum's second trip.  Every row's d, info and gradient
    have the bits they have alone, rows 64 .. 69 included; loss = float32 of minus the float64 sum of d in ascending rows"""
    ops = _ops()
    names = [CYCLE_10K[i % len(CYCLE_10K)] for i in range(70)]
    assert sum(G.has_segment(n) for n in names[64:] if n != "short") >= 3 and "short" in names[64:]
    L = 9001
    P = L + 37
    x, y, lengths = LG._batch(names, P)
    d2, info = ops.stoi(x[:, :L], y[:, :L], lengths=lengths, fs=10000, both=True, return_info=True)
    assert d2.shape == (70, 2) and info.shape == (70, 3)
    for b, n in enumerate(names):
        if n == "short":
            assert info[b].tolist() == [0, 0, 0] and d2[b].tolist() == [1e-5, 1e-5]
            continue
        da, ia = SG._alone(n)
        assert torch.equal(_i64(d2[b]), _i64(da)) and torch.equal(info[b], ia), (b, n)
        assert info[b].tolist() == [R.reference(n)[k] for k in ("frames", "kept", "segments")]
    for which in (1, 2):
        wide = y.clone().requires_grad_(True)
        loss, d = ops.stoi_loss(wide[:, :L], x[:, :L], lengths=lengths, fs=10000, extended=which == 2, return_scores=True)
        loss.backward()
        g = wide.grad
        assert d.shape == (70,) and g.shape == (70, P) and bool(torch.isfinite(g).all())
        assert torch.equal(_i64(d), _i64(d2[:, which - 1]))
        total = 0.0
        for b, n in enumerate(names):
            assert torch.count_nonzero(g[b, lengths[b]:]).item() == 0
            total += float(d[b])
            if n == "short":
                assert float(d[b]) == 1e-5 and torch.count_nonzero(g[b]).item() == 0
                continue
            _, da, ga = LG._alone(n, which)
            assert torch.equal(_i64(d[b:b + 1]), _i64(da)), (b, n)
            assert torch.equal(g[b, :lengths[b]], ga), (b, n)
        print("70 rows, which %d: loss %.9g, -sum of d %.17g" % (which, float(loss.detach()), -total))
        assert float(loss.detach()) == float(np.float32(-total))
