"""CPU tests of the video front-end's host side: the frame-rate map (``ops.lip_out_frames`` / ``lip_frame_starts``) against
a float-free brute-force restatement and the frame counts recorded in the reference's data, the float64 restatement
(tests/lip_ref.py) against the literal scipy expression of the reference, and the exported symbols.  The oracles of
test_lip_gpu.py's cases past one loop trip: the one-hot utterance's closed form, its derived bound (1.368e-4 level) held by
a float32 stand-in (2.39e-5) and broken by four planted mistakes, the 600-frame utterance against restatements that stop
after one or two trips, the loops and grids the many-utterance cases reach, and rates that drop frames."""
import os

import numpy as np
import pytest
import torch

import lip_ref as R
from conftest import GOLDEN


def brute_start(i, p, q):
    """round_half_away(i p / q) for non-negative integers without a division: the smallest s with 2 q s + q > 2 i p,
    i.e. s > i p / q - 1/2."""
    s = 0
    while 2 * q * s + q <= 2 * i * p:
        s += 1
    return s


def test_frame_map_matches_brute_force_and_is_monotone():
    from avvad import ops
    assert ops.lip_rate() == (25, 12) and R.rate() == (25, 12)
    starts = ops.lip_frame_starts(400)
    assert starts == [brute_start(i, 25, 12) for i in range(401)] == R.frame_starts(400)
    assert starts[:8] == [0, 2, 4, 6, 8, 10, 13, 15] and starts[6] == 13          # 12.5 -> 13: the tie rounds away from zero
    for N in range(401):
        assert ops.lip_out_frames(N) == starts[N]
        assert ops.lip_frame_starts(N) == starts[:N + 1]
    d = np.diff(starts)
    assert d.min() >= 1 and set(d.tolist()) == {2, 3}                                # every input frame is shown
    assert R.frame_map(13).tolist() == np.repeat(np.arange(13), d[:13]).tolist() and len(R.frame_map(13)) == starts[13]


def test_other_rates():
    from avvad import ops
    # 25 frames/s video, 10 ms hop at 16 kHz: exactly four output frames per input frame
    assert ops.lip_rate(16000, 160, 25) == (4, 1)
    assert ops.lip_frame_starts(5, 16000, 160, 25) == [0, 4, 8, 12, 16, 20] and ops.lip_out_frames(7, 16000, 160, 25) == 28
    # floats that hold integers, and a rate below one (frames are dropped, the map stays monotone)
    assert ops.lip_rate(16e3, 256, 30.0) == (25, 12)
    p, q = ops.lip_rate(8000, 512, 25)
    assert (p, q) == (5, 8)
    s = ops.lip_frame_starts(50, 8000, 512, 25)
    assert s == [brute_start(i, p, q) for i in range(51)] and np.diff(s).min() >= 0
    for fs, hop, fps in ((16000, 256, 30), (16000, 160, 25), (44100, 512, 24)):
        p, q = ops.lip_rate(fs, hop, fps)
        s = ops.lip_frame_starts(300, fs, hop, fps)
        assert s == [brute_start(i, p, q) for i in range(301)]
        if p >= q:
            assert np.diff(s).min() >= 1


def test_recorded_frame_counts_of_the_reference_data():
    """(N, stored T) of the nine utterances under the reference's data/subset: the stored length is min(T_video, T_label),
    and it equals the label count in all nine, so T_video >= stored T.  round-half-away satisfies that, floor does not."""
    from avvad import ops
    z = np.load(os.path.join(GOLDEN, "lip_frames.npz"))
    n_in, stored, labels, samples = z["n_in"], z["stored_t"], z["label_frames"], z["wav_samples"]
    assert len(n_in) == 9 and np.array_equal(stored, labels)
    assert [ops.target_frames(int(L))[1] for L in samples] == labels.tolist()
    assert all(ops.lip_out_frames(int(n)) >= int(t) for n, t in zip(n_in, stored))
    floor = [int(n) * 25 // 12 for n in n_in]
    assert any(f < int(t) for f, t in zip(floor, stored))
    assert 152 * 25 // 12 == 316 < 317 <= ops.lip_out_frames(152)


def test_restatement_against_the_scipy_expression():
    from scipy.fftpack import idct
    coef = R.synthetic_coef(40, seed=0).astype(np.float64)
    A = np.zeros((40, 67, 67))
    for n in range(40):                                              # create_video_train_files_upsampled.py:147-150
        A[n] = idct(idct(coef[n].reshape(67, 67)).T).T
    ref = np.stack([np.rot90((a - A.min()) / (A.max(axis=(-2, -1)) - A.min(axis=(-2, -1))).max() * 255.0, 3) for a in A])   # :156-157
    got = R.frames(coef, quantize=False)
    err_idct = np.abs(R.idct2(coef) - A).max() / np.abs(A).max()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("idct2 vs scipy %.2e relative, frames %.2e relative" % (err_idct, err))
    assert err_idct <= 1e-12 and err <= 1e-12
    # the global minimum with the largest PER-FRAME range: values above 255 occur before the clip
    assert got.min() == 0.0 and got.max() > 255.0
    q = R.frames(coef)
    assert q.max() == 255.0 and q.min() == 0.0 and np.array_equal(q, np.trunc(q))
    assert np.array_equal(q, np.trunc(np.clip(ref, 0, 255)))


def test_rot90_identity_and_frame_repeat():
    rng = np.random.default_rng(3)
    V = rng.standard_normal((3, 67, 67))
    out = R.rot90_3(V)
    for n in range(3):
        assert np.array_equal(out[n], np.rot90(V[n], 3))
    i, j = 5, 60
    assert out[1][i][j] == V[1][66 - j][i]
    # the rotation inside the product: out = C X^T C'^T with C' = C with its rows reversed
    coef = R.synthetic_coef(2, seed=1).astype(np.float64)
    C = R.dct_matrix()
    X = coef.reshape(2, 67, 67)
    fused = np.einsum("ib,nab,ja->nij", C, X, C[::-1], optimize=True)
    assert np.abs(fused - R.rot90_3(R.idct2(coef))).max() <= 1e-9 * np.abs(fused).max()
    full = R.decode(coef)
    assert full.shape == (4, 67, 67) and np.array_equal(full[0], full[1]) and np.array_equal(full[2], full[3])
    assert R.decode(coef, n_out=3).shape[0] == 3 and R.decode(coef, n_out=9).shape[0] == 4


def test_constant_frames_are_written_as_zero():
    coef = np.zeros((4, 67 * 67))
    coef[:, 0] = 3.0                                                 # only the DC term: every frame is the constant 3
    A = R.idct2(coef)
    assert np.abs(A - 3.0).max() <= 1e-12 and (A.max(axis=(-2, -1)) - A.min(axis=(-2, -1))).max() <= 1e-12
    coef[:, 0] = 0.0
    out = R.decode(coef, quantize=False)
    assert out.shape == (8, 67, 67) and not out.any() and np.isfinite(out).all()
    assert R.decode(np.zeros((0, 67 * 67))).shape == (0, 67, 67)


def test_symbols_are_exported_and_declared():
    from avvad import _lib as L
    from avvad import ops
    assert {"avvad_lip_decode_workspace", "avvad_lip_decode"} <= set(L.SIGNATURES)
    h = L.lib()
    assert hasattr(h, "avvad_lip_decode") and h.avvad_abi_version() == 3
    import ctypes as C
    d = L.LipDesc(2, 150, 300, 313, 67, 67, 25, 12, 1, 1e-8)
    need = h.avvad_lip_decode_workspace(C.byref(d))
    assert need >= 300 * (2 * 4 + 16) + 68 * 68 * 4
    for field, bad in (("B", 0), ("rows", 0), ("T", 0), ("W", 64), ("H", 66), ("p", 0), ("q", -1), ("n_max", 0)):
        e = L.LipDesc(2, 150, 300, 313, 67, 67, 25, 12, 1, 1e-8)
        setattr(e, field, bad)
        assert h.avvad_lip_decode_workspace(C.byref(e)) == 0, field
        # bad shapes are refused before anything is launched (all pointers are checked first, so dummies will do)
        one = C.c_void_p(256)
        assert h.avvad_lip_decode(one, one, one, None, one, one, None, None, None, C.byref(e), one, 1 << 30, None) == -1, field
    for name in ("lip_decode", "lip_out_frames", "lip_frame_starts", "lip_rate"):
        assert callable(getattr(ops, name))
    from packages.processing import video
    assert callable(video.decode_ntcd_frames)
    from avvad import train as TR
    for name in ("AVFiles", "av_file_step", "read_av_files", "av_file_stats"):
        assert hasattr(TR, name)


# ------------------------------------------------------------------------------------------ the oracles of test_lip_gpu.py
def test_onehot_utterance_closed_form_bound_and_mutants():
    """The one-hot utterance of test_lip_gpu.py: its closed form is the restatement, the derived bound (1.37e-4 level) holds
    for a float32 stand-in of the kernel's formula and not for four planted mistakes."""
    coef, pairs, amp = R.onehot_coef()
    N = len(pairs)
    assert N == 189 and N % 4 == 1 and coef.shape == (N, 67 * 67) and (coef != 0).sum() == N
    assert {a for a, _ in pairs} == {b for _, b in pairs} == set(range(67))
    assert {(a, b) for a in R.TILE_EDGES for b in R.TILE_EDGES} <= set(pairs) and pairs[-1] == (0, 0)
    exact = R.onehot_frames64(pairs, amp)
    # the index convention: A[ii][j] = x C[ii][b] C[66 - j][a] is what the restatement computes from the coefficients
    assert np.abs(exact - R.frames(coef, quantize=False)).max() <= 1e-9
    dc = exact[-1]
    assert np.ptp(dc) <= 1e-9 and 0 < dc.mean() < 255 and exact.min() == 0.0 and exact.max() > 254.0   # constant, utterance not
    bound = R.onehot_bound(pairs, amp)
    got = R.onehot_float32(coef)
    err = np.abs(got - exact).max()
    print("one-hot: float32 stand-in max |d| = %.3e level, derived bound %.3e" % (err, bound))
    assert 1.0e-4 < bound < 2.0e-4 and 0 < err <= bound
    for mutant in ("entry", "reverse", "pad", "transpose"):
        bad = np.abs(R.onehot_float32(coef, mutant) - exact).max()
        print("  mutant %-9s max |d| = %.3e" % (mutant, bad))
        assert bad > 100 * bound, mutant
    # quantised: the float64 reference alone excuses well under the 3 % cap, and the stand-in passes the excuse rule
    near = np.abs(exact - np.rint(exact)) <= bound
    print("one-hot: %.4f %% of the pixels excusable" % (100 * near.mean()))
    assert near.mean() <= 0.03
    differ = R.quantise(got) != R.quantise(exact)
    assert np.all(near[differ])
    assert np.any((R.quantise(R.onehot_float32(coef, "entry")) != R.quantise(exact)) & ~near)


def test_long_utterance_needs_every_trip_of_the_frame_loop():
    coef = R.long_utterance()
    A = R.idct2(coef)
    lo, rg = A.min(axis=(-2, -1)), A.max(axis=(-2, -1)) - A.min(axis=(-2, -1))
    assert A.shape[0] == 600 and int(lo.argmin()) == R.LONG_LO >= 256 and int(rg.argmax()) == R.LONG_RANGE >= 512
    assert lo[:256].min() > lo.min() and rg[:256].max() < rg.max()
    assert np.delete(lo, R.LONG_LO).min() > lo.min() and np.delete(rg, R.LONG_RANGE).max() < rg.max()
    ref = R.decode(coef, quantize=False, **R.ONE)
    assert ref.shape[0] == 600 and ref.min() == 0.0 and (ref <= 255.0).mean() > 0.9                # the clip does not hide the levels
    tol = R.tolerance(coef)
    assert 0 < tol <= 0.01
    for first in (256, 512):                                     # one trip, two trips
        bad = R.decode_first_frames_only(coef, first, **R.ONE)
        assert np.abs(bad - ref).max() > 100 * tol
        near = np.abs(ref - np.rint(ref)) <= tol
        assert ((R.quantise(bad) != R.quantise(ref)) & ~near).any()


def grid_x(n_max, B, cus=256):
    """lip_frames' grid: workgroups per utterance (csrc/lip.hip, avvad_lip_decode)"""
    return max(1, min(-(-n_max // 4), cus // B))


def test_many_utterance_cases_reach_their_loops():
    # statistics add: utterances in three trips of the wave loop, frames in three trips of the lane loop
    n_in = R.stats_add_counts()
    sums = np.arange(1, sum(n_in) + 1, dtype=np.float64)         # any per-frame partials
    whole = R.add_model(sums, n_in)
    assert whole == sums.sum()
    assert R.add_model(sums, n_in, max_waves=16) != whole and R.add_model(sums, n_in, max_waves=32) != whole
    assert R.add_model(sums, n_in, max_lane_trips=1) != whole and R.add_model(sums, n_in, max_lane_trips=2) != whole
    # count loop: more utterances than lip_add has threads, and no CU left per utterance
    n_in = R.count_counts()
    assert len(n_in) == 1030 > 1024 and set(n_in) == {1, 2} and grid_x(max(n_in), len(n_in)) == 1 and 256 // len(n_in) == 0
    assert sum(n_in[:1024]) != sum(n_in)
    # ragged multi-trip: two workgroups, stride 8, two trips, none of them whole
    n_in = R.ragged_counts()
    assert len(n_in) == 128 and set(n_in) == {9, 10, 11, 12, 13} and grid_x(max(n_in), 128) == 2
    assert all(-(-n // 8) == 2 and n % 8 for n in n_in)
    # the one-hot batch under a cap of 4 CUs: one workgroup per utterance, 48 trips with a prefetch each
    assert grid_x(189, 4, cus=4) == 1 and -(-189 // 4) == 48


@pytest.mark.parametrize("fps_in", R.RATES)
def test_rates_below_one_drop_frames_that_still_normalise(fps_in):
    from avvad import ops
    p, q = R.rate(hop=256, fps_in=fps_in)
    assert (p, q) == ops.lip_rate(16000, 256, fps_in) == {25: (5, 2), 50: (5, 4), 100: (5, 8), 125: (1, 2)}[fps_in]
    for N in (0, 1, 2, 37, 50):
        s = R.frame_starts(N, hop=256, fps_in=fps_in)
        assert s == [brute_start(i, p, q) for i in range(N + 1)] == ops.lip_frame_starts(N, 16000, 256, fps_in)
        fm = R.frame_map(N, hop=256, fps_in=fps_in)
        assert len(fm) == s[N] == ops.lip_out_frames(N, 16000, 256, fps_in) and np.all(np.diff(fm) >= 0)
    if fps_in == 125:
        assert R.frame_starts(4, hop=256, fps_in=125) == [0, 1, 1, 2, 2]          # 0.5 -> 1, 1.5 -> 2: ties away from zero
    for coef in R.rate_utterances(fps_in):
        N = coef.shape[0]
        gone = R.dropped_frames(N, hop=256, fps_in=fps_in)
        assert (len(gone) > 0) == (p < q)
        if p >= q:
            continue
        A = R.idct2(coef)
        lo, rg = A.min(axis=(-2, -1)), A.max(axis=(-2, -1)) - A.min(axis=(-2, -1))
        assert int(lo.argmin()) in gone and int(rg.argmax()) in gone and int(lo.argmin()) != int(rg.argmax())
        ref = R.decode(coef, quantize=False, hop=256, fps_in=fps_in)
        bad = R.decode_seen_frames_only(coef, hop=256, fps_in=fps_in)
        assert np.abs(bad - ref).max() > 100 * R.tolerance(coef)


def test_cpu_tensors_raise():
    from avvad import _lib as L
    from avvad import ops
    coef = torch.zeros(1, 3, 67 * 67)
    with pytest.raises(L.AvvadError):
        ops.lip_decode(coef, [3])
    with pytest.raises(L.AvvadError):
        ops.lip_decode(coef.double(), [3])
    from packages.processing import video
    with pytest.raises(L.AvvadError):
        video.decode_ntcd_frames(np.zeros((3, 67 * 67)), device="cpu")
