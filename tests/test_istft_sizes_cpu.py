"""The CPU companion of tests/test_istft_sizes_gpu.py: the cases meet the conditions the GPU tests rely on (a second trip
that exists, is compared and is not compared against zeros; ``E_cpu32 > 0``; a long last row), the float32 yardstick
passes the very checks the GPU result has to pass, and a kernel that stops after one trip of ``istft_sizes_ref.TRIP``
elements -- or takes its second trip from an index one row off -- is rejected by them."""
import numpy as np
import pytest

import istft_ref as R
import istft_sizes_ref as Z
import sisdr_ref as S

FORWARD = [(False, 0), (True, 0), (False, 2)]


def _rejected(check, *a, **k):
    with pytest.raises(AssertionError):
        check(*a, **k)


def test_the_trip_is_grid1s():
    """frames::grid1 caps a launch at 4096 workgroups; the four loops run 256 threads each"""
    import os
    import re
    from conftest import PKG
    text = open(os.path.join(PKG, "csrc", "frames.h")).read()
    cap = re.search(r"int grid1\(long n\) \{ long b = \(n \+ 255\) / 256; .*\(b > (\d+) \? (\d+) :", text)
    assert cap and int(cap.group(1)) == int(cap.group(2)) and int(cap.group(1)) * 256 == Z.TRIP == 1048576


@pytest.mark.parametrize("center,mode", FORWARD)
def test_batched_forward_case_and_a_kernel_of_one_trip(center, mode):
    case = Z.forward_case(Z.N_FFT, Z.HOP, Z.FRAMES, center, mode, seed=7)
    B, pitch = len(Z.FRAMES), case["pitch"]
    assert pitch == (66304 if center else 67328) and B * pitch == (1060864 if center else 1077248)
    assert case["frames"][15] == 260 and 15 * pitch < Z.TRIP < B * pitch                 # the second trip lies in row 15 alone
    assert B * max(Z.FRAMES) == 4160 and (-(-4160 // 128), -(-Z.N_FFT // 128)) == (33, 8)
    tail = Z.reference_past_trip(case, 15)
    assert tail.size == B * pitch - Z.TRIP == (12288 if center else 28672) and np.count_nonzero(tail) == tail.size
    assert all(r is None or r["e32"] > 0 for r in case["rows"])
    assert [r is None for r in case["rows"]] == [n == 0 for n in case["natural"]]
    y32 = Z.yardstick(case)
    worst = Z.check_forward(y32, case)
    assert 0 < worst <= 1.0
    _rejected(Z.check_forward, Z.stops_after_one_trip(y32), case)
    _rejected(Z.check_forward, Z.second_trip_off_by(y32, pitch), case)                   # row 15 written from row 14's index


@pytest.mark.parametrize("n_fft,hop,T", Z.LONG)
def test_long_utterance_case_and_a_kernel_of_one_trip(n_fft, hop, T):
    case = Z.forward_case(n_fft, hop, (T,), False, 0, seed=n_fft + hop)
    assert case["pitch"] == {64: 1049648, 1024: 1050368}[n_fft] > Z.TRIP
    if n_fft == 64:
        assert (-(-T // 128), -(-n_fft // 128)) == (513, 1)
    tail = Z.reference_past_trip(case, 0)
    assert tail.size == case["pitch"] - Z.TRIP and np.count_nonzero(tail) == tail.size
    assert case["rows"][0]["e32"] > 0
    y32 = Z.yardstick(case)
    Z.check_forward(y32, case)
    _rejected(Z.check_forward, Z.stops_after_one_trip(y32), case)
    _rejected(Z.check_forward, Z.second_trip_off_by(y32, hop), case)                     # (B = 1: off by one frame)


@pytest.mark.parametrize("which", ["A", "B"])
def test_adjoint_case_and_a_kernel_of_one_trip(which):
    case = Z.adjoint_case(which)
    F = Z.N_FFT // 2 + 1
    assert case["ref"].shape == (16, 260, F) and case["ref"].size == 2134080 and case["frames"][15] == 260
    Lq = 259 * Z.HOP + Z.N_FFT
    assert 16 * Lq == 1077248 and 15 * Lq < Z.TRIP                                       # overlap_add_adjoint's second trip: q[15]
    tail = Z.past_trip(case["ref"])
    assert tail.size == 1085504 and 2 * np.count_nonzero(tail) >= tail.size
    print("adjoint %s: %d of %d reference values past the first trip are non-zero" % (which, np.count_nonzero(tail), tail.size))
    if which == "B":
        nat = [R.istft_length(nf, Z.N_FFT, Z.HOP, True) for nf in Z.FRAMES]
        assert [b for b in range(16) if case["lengths"][b] < nat[b]] == [6, 15] and len(set(case["scale"].tolist())) == 16
    e, e32 = S.check_dmask(lambda c: c["y32"], case)
    assert e == e32 > 0
    _rejected(S.check_dmask, lambda c: Z.stops_after_one_trip(c["y32"]), case)
    _rejected(S.check_dmask, lambda c: Z.second_trip_off_by(c["y32"], F), case)          # GEMM row x - 1 in place of x
    _rejected(S.check_dmask, lambda c: Z.second_trip_off_by(c["y32"], 260 * F), case)    # batch row b - 1 in place of b
    _rejected(S.check_dmask, Z.adjoint_with_q_of_one_trip, case)                         # overlap_add_adjoint of one trip


def test_adjoint_case_with_a_row_of_no_frames():
    case = S.cached_istft_case(64, 16, (9, 0, 4), 2, True, 5)
    assert case["lengths"][1] == 0 and not case["ref"][1].any() and np.isnan(case["spec"][1]).all()
    got = S.dmask_closed(case)
    assert np.abs(got - case["ref"]).max() <= 1e-12 * np.abs(case["ref"]).max()
    S.check_dmask(S.dmask_closed, case)
    _rejected(S.check_dmask, lambda c: S.dmask_closed(c, form=S.MUTANTS["rows t >= n_frames not zeroed"]), case)


def test_basis_case_and_a_basis_of_one_trip():
    """2048 / 512: the inverse basis has 2052 x 2048 elements; written for one trip only, its rows c >= 512 (bins f >= 256)
    are missing, which is the inverse of a spectrum that is zero from bin 256 on"""
    n_fft, hop, frames = 2048, 512, (3, 1)
    case = Z.forward_case(n_fft, hop, frames, False, 0, seed=9)
    assert Z.TRIP // n_fft == 512 and all(r["e32"] > 0 for r in case["rows"])
    y32 = Z.yardstick(case)
    Z.check_forward(y32, case)
    cut = np.zeros_like(y32)
    for b, nf in enumerate(frames):
        Sb = (case["spec"][b, :nf, :, 0] + 1j * case["spec"][b, :nf, :, 1]).astype(np.complex128)
        Sb[:, 256:] = 0
        cut[b, :case["natural"][b]] = R.istft32_gemm(Sb, n_fft, hop, length=case["natural"][b])
    _rejected(Z.check_forward, cut, case)
    adj = S.cached_istft_case(n_fft, hop, frames, 2, True, 10)
    e, e32 = S.check_dmask(lambda c: c["y32"], adj)
    assert e == e32 > 0


def test_chain_case_crosses_the_trip():
    case = Z.chain_case()
    assert case["mask"].shape == (16, 185, 513) and case["mask"].size == 1518480 > Z.TRIP
    tail = Z.past_trip(case["ref"])
    assert 2 * np.count_nonzero(tail) >= tail.size
    e, e32 = S.check_chain(lambda c: (c["loss64"], c["y32"]), case)
    assert e == e32 > 0
    _rejected(S.check_chain, lambda c: (c["loss64"], Z.stops_after_one_trip(c["y32"])), case)


def _closed32(case, rows=None):
    loss, ratios, grad, _, _ = S.sisdr_closed(case["est"], case["ref"], case["lengths"], case["head"], case["tail"], dtype=np.float32)
    if rows is not None:
        loss = -float(np.nansum(ratios[:rows]))
    return loss, ratios, grad


def test_loss_case_and_a_workgroup_of_one_stride():
    from avvad import ops
    case = Z.loss_case(ops.SCORE_CHUNK)
    lengths = case["lengths"]
    assert len(lengths) == 300 and lengths[:3] == [300, 307, 314] and max(lengths) == lengths[Z.LOSS_LONG] == ops.SCORE_CHUNK + 77
    assert lengths[Z.LOSS_ZERO_LENGTH] == 0 and 0 < lengths[Z.LOSS_EMPTY_WINDOW] <= Z.LOSS_HEAD + Z.LOSS_TAIL
    assert min(Z.LOSS_EMPTY_WINDOW, Z.LOSS_ZERO_LENGTH, Z.LOSS_LONG) >= 256
    others = [n for b, n in enumerate(lengths) if b not in (Z.LOSS_EMPTY_WINDOW, Z.LOSS_ZERO_LENGTH, Z.LOSS_LONG)]
    assert min(others) == 300 and max(others) <= 699
    for b, n in enumerate(lengths):
        assert np.isnan(case["est"][b, n:]).all() and np.isfinite(case["est"][b, :n]).all()
    live = [b for b, n in enumerate(lengths) if n > 0]
    assert np.isfinite(case["ratios64"][live]).all() and np.isnan(case["ratios64"][Z.LOSS_ZERO_LENGTH]).all()
    S.check_sisdr(_closed32, case)
    _rejected(S.check_sisdr, lambda c: _closed32(c, rows=256), case)                     # rows >= 256 left out of the loss sum
