"""CPU tests of the encoder oracle (tests/encoder_ref.py): the restatement against ``oracle.wavenet``, TAU against the
measured float32 spread, the cap on ambiguous units, every case of tests/test_encoder_gpu.py with the float32 CPU oracle in
the place of the HIP path (the bounds are within reach of a correct float32 evaluation, and the harness works), the case
table against the restated form choices of csrc/wavenet.hip, mutants of the stand-in that ``check_encoder`` must reject, and
the pool-bin cover the tail-backward kernels rely on, exhaustively."""
import numpy as np
import pytest
import torch

import encoder_ref as R
import head_ref as H
from oracle import wavenet as ow

TAG = "cpu32"


def _one_thread(fn):
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn()
    finally:
        torch.set_num_threads(n)


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ["E1r", "E2", "E6", "E6n", "T1-48", "T2", "T3"])
def test_restatement_equals_the_oracle_in_float64(name):
    """out, every gradient and the block inputs s_i against ``oracle.wavenet.encode``; out against ``encode_loops`` (which
    pins tap order, residual crop and pool bins without a library call)"""
    inp = R.inputs(name)
    ref = R.reference(name)
    sd = {k: v.double().requires_grad_(True) for k, v in inp.params.items()}
    wave = inp.wave.double().requires_grad_(True)
    out, inter = ow.encode(sd, wave, inp.cfg, return_intermediates=True)
    ((out * inp.G.double()).sum() * R.UPSTREAM).backward()
    assert float((ref.out - out.detach()).abs().max()) <= 1e-14 * max(1.0, float(out.detach().abs().max()))
    for i in range(len(inp.cfg["dilations"])):
        assert float((ref.pre[("s", i)] - inter[i].detach()).abs().max()) <= 1e-13
    assert tuple(ref.pre[("b", 0)].shape[1:]) == (inp.cfg["en_bottleneck_width"], R.lengths(name)[-1])
    for k, v in sd.items():
        assert float((ref.grads[k] - v.grad).abs().max()) <= 1e-12 * max(1.0, float(v.grad.abs().max())), k
    assert float((ref.grads["wave"] - wave.grad).abs().max()) <= 1e-12 * max(1.0, float(wave.grad.abs().max()))
    with torch.no_grad():
        loops = ow.encode_loops({k: v.detach() for k, v in sd.items()}, wave.detach(), inp.cfg)
    assert float((ref.out - loops).abs().max()) <= 1e-12 * max(1.0, float(loops.abs().max()))


@pytest.mark.parametrize("name", ["E1r", "E2", "E6n", "T2"])
def test_float32_stand_in_is_the_oracle_bit_for_bit(name):
    inp = R.inputs(name)
    got = R.run(name, torch.float32, keep_pre=True)
    with torch.no_grad():
        out, inter = _one_thread(lambda: ow.encode(inp.params, inp.wave, inp.cfg, return_intermediates=True))
    assert torch.equal(got.out, out)
    for i in range(len(inp.cfg["dilations"])):
        assert torch.equal(got.pre[("s", i)], inter[i])


def test_a_mutant_leaves_the_forward_alone():
    """the mutants are wrong BACKWARDS: out is the unmutated stand-in's, bit for bit"""
    for mutant, name in (("taps_swapped", "E2"), ("residual_wrong_end", "E2"), ("wgrad_drops_last_tile", "E3"),
                         ("causal_ignores_seq_32", "E5"), ("pool_end_rounded_down", "E2"), ("pool_three_bin_window", "T2")):
        assert torch.equal(R.run(name, torch.float32, mutant=mutant).out, R.run(name, torch.float32).out), mutant


# ------------------------------------------------------------------------------------------ TAU and the ambiguous units
def test_tau_is_eight_times_the_float32_spread():
    """max |pre_float32 - pre_float64| over the three ReLU families of every case; the figures of encoder_ref's docstring"""
    spread = {}
    for name in R.CASES:
        ref, r32 = R.reference(name), R.run(name, torch.float32, keep_pre=True)
        assert set(ref.pre) == set(r32.pre)
        spread[name] = max(float((r32.pre[k].double() - ref.pre[k]).abs().max()) for k in ref.pre)
        flips = sum(int(((r32.pre[k] > 0) != (ref.pre[k] > 0)).sum()) for k in ref.pre)
        print("%-7s float32 spread %.2e, ReLU decisions that differ %d, ambiguous units %d" % (
            name, spread[name], flips, len(R.ambiguous(name))))
    worst = max(spread.values())
    print("TAU = %.1e = %.1f x the worst spread %.2e (%s)" % (R.TAU, R.TAU / worst, worst, max(spread, key=spread.get)))
    assert R.TAU >= 8.0 * worst
    assert R.TAU <= 1e-5            # (and not so wide that the ambiguous lists stop being short)


@pytest.mark.parametrize("name", list(R.CASES))
def test_ambiguous_units_are_few_and_sorted(name):
    A, pre = R.ambiguous(name), R.reference(name).pre
    assert len(A) <= R.MAX_AMBIGUOUS
    mags = [abs(float(pre[(f, i)][b, c, t])) for f, i, b, c, t in A]
    assert mags == sorted(mags) and all(m < R.TAU for m in mags)
    assert len(A) == sum(int((x.abs() < R.TAU).sum()) for x in pre.values())


# ------------------------------------------------------------------------------------------ the float32 oracle under the checks
@pytest.mark.parametrize("name", list(R.CASES))
def test_float32_oracle_passes_at_a_quarter_of_the_bounds(name):
    before = H.WORST.pop((TAG, R.FAMILY), None)
    assert R.check_encoder(R.encoder_fp32, name, tag=TAG) == ()
    ratio, what = H.WORST[(TAG, R.FAMILY)]              # the worst of this case alone
    if before is not None and before[0] > ratio:
        H.WORST[(TAG, R.FAMILY)] = before
    assert ratio <= 0.25, (ratio, what)


@pytest.mark.parametrize("name,frozen", [("E2", ("wave",)), ("E6", ("en_dilation_layer_stack.1.weight", "en_dense_layer_stack.1.bias"))])
def test_float32_oracle_passes_with_a_subset(name, frozen):
    assert R.check_encoder(R.encoder_fp32, name, frozen=frozen, tag=TAG) == ()
    with pytest.raises(AssertionError, match="is frozen and has a gradient"):
        R.check_encoder(lambda inp, fr: R.encoder_fp32(inp), name, frozen=frozen, tag=None)


def test_float32_oracle_accumulates():
    assert R.check_encoder(lambda inp, fr: R.encoder_fp32(inp, fr, passes=2), "E1r", tag=TAG, label="two passes", passes=2) == ()
    with pytest.raises(AssertionError, match="d/d"):       # one pass is not two
        R.check_encoder(R.encoder_fp32, "E1r", tag=None, passes=2)


# ------------------------------------------------------------------------------------------ what the case table reaches
def test_case_table_reaches_what_it_claims():
    L = R.lengths
    C = R.CASES
    # E1 / E1r: one tile / one tile + one sample in front of the pool; Bn = 32: tail forward <1>, tail backward MFMA
    assert L("E1")[-1] == 32 and L("E1r")[-1] == 33
    assert R.tail_bwd_form(33, 32, 32, 4) == "MFMA" and C["E1"]["Bn"] % 128 != 0
    # E2: dilation 64 > tile, an odd dilation, no layer length a multiple of 32, odd pitches, overlapping bins, PAIR
    Ls = L("E2")
    assert Ls == [299, 298, 296, 232, 229, 197] and all(n % 32 for n in Ls) and sum(n % 2 for n in Ls) >= 3
    assert 64 in C["E2"]["dil"] and 3 in C["E2"]["dil"] and 197 % 7 != 0
    bins = R.pool_bins(197, 7)
    assert any(bins[p][1] > bins[p + 1][0] for p in range(6))
    assert R.tail_bwd_form(197, 32, 256, 7) == "PAIR"
    assert R.tail_bwd_form(197, 32, 256, 7, wn_no_tail_pair=1) == "FUSED"
    assert R.tail_bwd_form(197, 32, 256, 7, wn_no_fused_tail=1) == "MFMA"
    assert R.tail_bwd_form(197, 32, 256, 7, any_grad=False) == "MFMA"
    # E3: 140 tiles per layer; fused backward 9 -> 8 workgroups (32 waves: > 4 tiles each), forward 35 -> 40 (160 waves)
    Ls = L("E3")
    for Lin, d in zip(Ls[:-1], C["E3"]["dil"]):
        assert 7 * R.cdiv(Lin - d, 32) == 140
        assert R.bwd_form(7, Lin - d) == ("OCC", 8) and R.cdiv(140, 16) == 9
        assert R.fwd_form(7, Lin, d) == ("OCC", 40) and R.cdiv(140, 4) == 35 and 40 * 4 > 140
        assert R.fwd_form(7, Lin, d, wn_grid=8) == ("OCC", 8)
        assert R.bwd_form(7, Lin - d, wn_bwd_t=1) == ("TRANSPOSED", 9) and R.bwd_form(7, Lin - d, wn_bwd_t=3) == ("RESIDENT", 9)
        assert R.bwd_form(7, Lin - d, wn_no_fused_wgrad=1)[0] == "UNFUSED" and R.bwd_form(7, Lin - d, any_grad=False)[0] == "UNFUSED"
        assert R.dx_form(7, Lin) == ("OCC", 40) and R.dx_form(7, Lin, wn_dx=1)[0] == "BUF"
        assert R.dx_form(7, Lin, wn_dx=3, wn_flat=1)[0] == "FLAT"
        assert [R.fwd_form(7, Lin, d, wn_flat=f)[0] for f in (1, 2, 3, 4, 5)] == ["FLAT", "BUF", "WIDE", "OCC", "DMA"]
    # E4: W0's stack, dilation 512, Lv = 103
    assert C["E4"]["dil"] == ow.W0["dilations"] and max(C["E4"]["dil"]) == 512 and L("E4")[-1] == 103
    # E5: more than 32 sequences; Bn = 64: tail forward <1>, tail backward MFMA
    assert C["E5"]["B"] > 32 and C["E5"]["Bn"] % 128 != 0 and R.tail_bwd_form(L("E5")[-1], 32, 64, 4) == "MFMA"
    # E6 / E6n: nothing of the MFMA shape; E6n has no bias
    assert not R.mfma_shape("E6") and not R.mfma_shape("E6n") and R.tail_bwd_form(102, 16, 40, 5) == "GENERIC"
    assert R.config("E6")["use_bias"] and not R.config("E6n")["use_bias"] and "en_causal_layer.bias" not in R.inputs("E6n").params
    # E7: MFMA blocks, GENERIC tail; E8: tail forward <4>, tail backward MFMA
    assert R.mfma_shape("E7") and R.tail_bwd_form(L("E7")[-1], 32, 48, 3) == "GENERIC"
    assert C["E8"]["Bn"] % 128 == 0 and R.tail_bwd_form(L("E8")[-1], 32, 128, 3) == "MFMA"
    # E9: both blocks on the dwordx4 forward, the second with a tap offset that is no multiple of 4
    Ls = L("E9")
    assert [R.fwd_form(2, Lin, d)[0] for Lin, d in zip(Ls[:-1], C["E9"]["dil"])] == ["WIDE", "WIDE"]
    assert Ls[1] >= 8192 and Ls[2] >= 8192 and C["E9"]["dil"][1] % 4 != 0
    assert [R.fwd_form(2, Ls[0], 512, wn_flat=f)[0] for f in (1, 2, 3, 4, 5)] == ["FLAT", "BUF", "WIDE", "OCC", "DMA"]
    # T: P > Lv goes to the generic tail backward whatever Bn and the options; P = Lv and P = 1 stay on the MFMA form
    for name, Lv in (("T1-256", 3), ("T1-32", 3), ("T1-48", 3), ("T2", 53), ("T3", 1)):
        assert L(name)[-1] == Lv and C[name]["P"] > Lv
        assert R.tail_bwd_form(Lv, 32, C[name]["Bn"], C[name]["P"]) == "GENERIC"
    assert C["T2"]["P"] == ow.W0["en_pool_kernel_size"]
    assert L("T4")[-1] == C["T4"]["P"] == 32 and C["T5"]["P"] == 1
    assert R.tail_bwd_form(32, 32, 32, 32) == "MFMA" and R.tail_bwd_form(32, 32, 32, 1) == "MFMA"
    # T6: more time tiles than one round of the fused tail backward takes (4 per workgroup, TAIL_MAXBLK workgroups), in
    # each of its three forms; the bins overlap, so the Lv % P shortcut is off
    assert L("T6")[-1] == 33 and 513 * R.cdiv(33, 32) == 1026 > 4 * R.TAIL_MAXBLK and 33 % 4 != 0
    assert R.pool_bins(33, 4) == [(0, 9), (8, 17), (16, 25), (24, 33)]
    assert R.tail_bwd_form(33, 32, 256, 4) == "PAIR"
    assert R.tail_bwd_form(33, 32, 256, 4, wn_no_tail_pair=1) == "FUSED"
    assert R.tail_bwd_form(33, 32, 256, 4, wn_no_fused_tail=1) == "MFMA"
    # the tail forward: E1 one bn-tile per wave, E8 four, E6 generic
    assert R.tail_fwd_form(1, 32, C["E1"]["Bn"], 4) == ("<1>", 1) and R.tail_fwd_form(2, 32, C["E8"]["Bn"], 3) == ("<4>", 2)
    assert R.tail_fwd_form(3, C["E6"]["R"], C["E6"]["Bn"], 5)[0] == "GENERIC"
    # E1r, E2 (the form cases): every layer of every case is short enough for a single int of tiles, long enough for a tile
    for name in ("E1r", "E2", "E3"):
        assert R.mfma_shape(name) and min(L(name)) >= 32


# ------------------------------------------------------------------------------------------ mutants
def _rejected_by_a_gradient(name, **kw):
    assert R.check_encoder(R.encoder_fp32, name, tag=None) == ()                 # the unmutated stand-in passes there
    with pytest.raises(AssertionError, match="d/d") as e:
        R.check_encoder(lambda inp, fr: R.encoder_fp32(inp, fr, **kw), name, tag=None)
    return str(e.value)


@pytest.mark.parametrize("mutant,name", [
    ("taps_swapped", "E2"), ("residual_wrong_end", "E2"), ("wgrad_drops_last_tile", "E3"), ("bgrad_drops_last_sample", "E1r"),
    ("causal_ignores_seq_32", "E5"), ("pool_end_rounded_down", "E2"),
    ("pool_three_bin_window", "T1-256"), ("pool_three_bin_window", "T1-32"), ("pool_three_bin_window", "T1-48"),
    ("pool_three_bin_window", "T2"), ("pool_three_bin_window", "T3")])
def test_mutant_is_rejected(mutant, name):
    msg = _rejected_by_a_gradient(name, mutant=mutant)
    print(msg.splitlines()[0])
    if mutant == "wgrad_drops_last_tile":
        assert "en_dilation_layer_stack.1.weight" in msg
    if mutant == "causal_ignores_seq_32":
        assert "en_causal_layer" in msg


@pytest.mark.parametrize("name", ["E2", "T4", "T5", "E4"])
def test_three_bin_window_is_enough_while_the_pool_is_no_longer_than_its_input(name):
    """the same mutant is no mutant where P <= Lv: the window the MFMA forms keep"""
    assert R.CASES[name]["P"] <= R.lengths(name)[-1]
    assert R.check_encoder(lambda inp, fr: R.encoder_fp32(inp, fr, mutant="pool_three_bin_window"), name, tag=None) == ()


def _unit_near(name, target, families=("z",)):
    """the unit of the given families whose |pre64| is nearest ``target``"""
    best = None
    for (fam, i), x in R.reference(name).pre.items():
        if fam in families:
            d = (x.abs() - target).abs()
            j = int(d.argmin())
            b, c, t = (int(v) for v in np.unravel_index(j, tuple(x.shape)))
            if best is None or float(d.reshape(-1)[j]) < best[0]:
                best = (float(d.reshape(-1)[j]), (fam, i, b, c, t))
    return best[1]


def test_a_flip_outside_the_ambiguous_units_is_rejected():
    """a unit with |pre| = 1e-3 switched the other way in the backward: a real error of the size a legitimate flip has.  It
    is not in ``ambiguous``, so the flip search cannot absorb it."""
    name = "E2"
    u = _unit_near(name, 1e-3)
    pre = abs(float(R.reference(name).pre[u[:2]][u[2:]]))
    assert 0.9e-3 < pre < 1.1e-3 and u not in R.ambiguous(name)
    msg = _rejected_by_a_gradient(name, flips=(u,), grad_only_flips=True)
    print(u, pre, msg.splitlines()[0])


def _visible(name, units):
    """the units whose flip alone takes a gradient of the float64 reference beyond its bound"""
    ref = R.reference(name).grads
    keys = sorted(ref)
    return [u for u in units if max(w for w, _ in R._errors(R.reference(name, (u,)).grads, ref, 1.0, keys)[0].values()) > 1.0]


def test_up_to_three_flips_inside_the_ambiguous_units_are_found():
    """the stand-in with 1, 2 and 3 ambiguous units on the other side: step 2 fails, the search names exactly those units"""
    name = "E3"
    vis = _visible(name, R.ambiguous(name))
    assert len(vis) >= 4, len(vis)
    for n in (1, 2, 3):
        S = tuple(vis[1:1 + n])                  # (not the first: the search must pass over units that do not help)
        got = R.check_encoder(lambda inp, fr: R.encoder_fp32(inp, fr, flips=S), name, tag=TAG, label="%d flips" % n)
        assert set(got) == set(S), (got, S)


def test_four_flips_are_rejected():
    """the cap: four visible flips, all inside ``ambiguous``, are one too many"""
    name = "E3"
    S = tuple(_visible(name, R.ambiguous(name))[:4])
    assert len(S) == 4
    _rejected_by_a_gradient(name, flips=S)


# ------------------------------------------------------------------------------------------ the pool-bin cover
def test_pool_bin_cover_exhaustively():
    """For every Lv <= 120, P <= 240 and every sample t: the bins [floor(p Lv / P), ceil((p + 1) Lv / P)) that contain t are
    exactly p0 .. p1 - 1 with p0 = floor(t P / Lv), p1 = ceil((t + 1) P / Lv) -- the loop of tail_bwd_dz_generic -- and the
    three-register window floor(t P / Lv) - 1 .. + 1 of the MFMA forms, with its membership test, finds all of them whenever
    P <= Lv -- the predicate of tail_bwd_form -- and loses some for 20 938 of the pairs with P > Lv."""
    lost_pairs = 0
    for Lv in range(1, 121):
        t = np.arange(Lv)[:, None]
        for P in range(1, 241):
            p = np.arange(P)[None, :]
            a, e = (p * Lv) // P, -((-(p + 1) * Lv) // P)
            member = (t >= a) & (t < e)                                   # (Lv, P) brute force
            p0, p1 = (t * P) // Lv, -((-(t + 1) * P) // Lv)
            assert np.array_equal(member, (p >= p0) & (p < p1)), (Lv, P)
            assert p0.min() >= 0 and p1.max() <= P and (p1 > p0).all()
            lost = member & (np.abs(p - p0) > 1)
            if P <= Lv:
                assert not lost.any(), (Lv, P)
                assert (p1 - p0).max() <= 2
            lost_pairs += bool(lost.any())
    assert lost_pairs == 20938
    # the issue's examples: Lv = 3, P = 5: sample 1 is in bins 1, 2, 3; W0's P = 60 at Lv = 53 loses 6 contributions
    assert [p for p, (a, e) in enumerate(R.pool_bins(3, 5)) if a <= 1 < e] == [1, 2, 3]
    M, Mw = R.pool_matrix(53, 60, torch.float64), R.pool_matrix(53, 60, torch.float64, "three_bin_window")
    assert int(((M != 0) & (Mw == 0)).sum()) == 6


def test_pool_matrix_is_the_adaptive_pool():
    x = torch.randn(2, 3, 53, dtype=torch.float64)
    for P in (1, 7, 53, 60, 200):
        ref = torch.nn.functional.adaptive_avg_pool1d(x, P)
        assert float((x @ R.pool_matrix(53, P, x.dtype).t() - ref).abs().max()) <= 1e-14


def test_zz_log_worst_ratios():
    R.log_worst(TAG)
