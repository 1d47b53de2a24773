"""CPU tests of the fusion-head oracle (tests/head_ref.py): the references against each other and against ``oracle/``, every
case of tests/test_head_gpu.py with the float32 CPU oracle in the place of the HIP path (the bounds are within reach of a
correct float32 evaluation, and the harness works), seeded mutants of that stand-in that the assertion functions must reject,
and the host-side validation of the count-sketch hashes."""
import numpy as np
import pytest
import torch

import head_ref as R
from oracle import fusion

TAG = "cpu32"


# ------------------------------------------------------------------------------------------ references against each other
def test_direct_sum_equals_the_naive_outer_product_sketch():
    for name in ("F4", "F4b", "F5", "F6"):
        inp = R.fusion_inputs(name)
        a, v = inp.a.double(), inp.v.double()
        y = R.mcb_direct(a, v, inp.h1, inp.s1.double(), inp.h2, inp.s2.double(), inp.D)
        ref = fusion.mcb_naive(a, v, inp.h1, inp.s1.double(), inp.h2, inp.s2.double(), inp.D)
        assert float((y - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), name


def test_direct_sum_equals_the_fft_form_on_a_dense_case():
    """D = 1024 behind 513 x 512 channels: every bucket is the sum of ~256 products, none is 0; the two forms agree to
    1e-12 max|y|, which is what lets the FFT form stand in for D >= 1000."""
    rng = np.random.default_rng(3)
    D = 1024
    h1, h2 = torch.from_numpy(rng.integers(0, D, 513)), torch.from_numpy(rng.integers(0, D, 512))
    s1, s2 = R._signs(rng, 513).double(), R._signs(rng, 512).double()
    a, v = R._rand(rng, 2, 513).double(), R._rand(rng, 2, 512).double()
    assert bool(R.reachable_buckets(h1, h2, D).all())
    direct = R.mcb_direct(a, v, h1, s1, h2, s2, D)
    fft = fusion.mcb(a, v, h1, s1, h2, s2, D)
    assert float(direct.abs().min()) > 0
    assert float((direct - fft).abs().max()) <= 1e-12 * float(direct.abs().max())


@pytest.mark.parametrize("name", ["F5", "F4"])
def test_direct_sum_has_exact_zeros_where_the_fft_form_has_not(name):
    """Why the direct sum is the reference of the sparse cases: at a bucket no (i, k) pair maps to it is exactly 0, the FFT
    form is ~1e-17 even in float64, and sign(1e-17) sqrt(1e-8) = +-1e-4 is not 0."""
    inp = R.fusion_inputs(name)
    a, v = inp.a.double(), inp.v.double()
    empty = ~R.reachable_buckets(inp.h1, inp.h2, inp.D)
    assert int(empty.sum()) > 0
    direct = R.mcb_direct(a, v, inp.h1, inp.s1.double(), inp.h2, inp.s2.double(), inp.D)
    fft = fusion.mcb(a, v, inp.h1, inp.s1.double(), inp.h2, inp.s2.double(), inp.D)
    assert bool((direct[..., empty] == 0).all())
    live = inp.a.abs().sum(-1) > 0                           # (row 1 has an all-zero audio frame: all of its y are 0)
    assert int((~live).sum()) == 1 and bool((direct[~live] == 0).all())
    assert bool((direct[live][..., ~empty] != 0).all())
    if name == "F5":
        assert int(empty.sum()) >= 10                        # almost all of its 16 buckets
        assert float(fft[..., empty].abs().max()) > 0
        z = torch.sign(fft) * torch.sqrt(fft.abs() + R.EPS)
        assert float(z[..., empty].abs().max()) > 0.99e-4


def test_restatements_equal_the_oracle_in_float64():
    """the mutable restatements differ from ``oracle/`` by their mutation alone"""
    inp = R.fusion_inputs("F4")
    for training in (True, False):
        y = R.mcb_direct(inp.a.double(), inp.v.double(), inp.h1, inp.s1.double(), inp.h2, inp.s2.double(), inp.D)
        res = []
        for which in ("oracle", "restated"):
            yl = y.clone().requires_grad_(True)
            w, b = inp.bn_w.double().requires_grad_(True), inp.bn_b.double().requires_grad_(True)
            rm, rv = inp.rm0.double().clone(), inp.rv0.double().clone()
            if which == "oracle":
                out = fusion.mcb_post(yl, w, b, rm, rv, R.EPS, training, R.MOMENTUM)
            else:
                out, rm, rv = R.post(yl, w, b, rm, rv, R.EPS, training, R.MOMENTUM, "restated")
            (out * inp.G.double()).sum().backward()
            res.append((out.detach(), yl.grad, w.grad, b.grad, rm, rv))
        for p, q in zip(*res):
            assert float((p - q).abs().max()) <= 1e-11 * max(1.0, float(p.abs().max()))
    li = R.lstm_inputs("L6")
    y0, g0 = R._lstm_run(li, torch.float64, (), None)
    y1, g1 = R._lstm_run(li, torch.float64, (), "restated")
    assert torch.equal(y0, y1) and all(float((g0[k] - g1[k]).abs().max()) <= 1e-13 for k in g0)
    for name in R.MASKED_BCE_CASES:
        mi = R.masked_bce_inputs(name)
        (l0, d0), (l1, d1) = R.masked_bce_eval(mi, torch.float64), R.masked_bce_eval(mi, torch.float64, "restated")
        assert abs(float(l0 - l1)) <= 1e-12 * abs(float(l0)) and float((d0 - d1).abs().max()) <= 1e-14
    bi = R.bce_2classes_inputs()
    p, q = R.bce_2classes_eval(bi, torch.float64), R.bce_2classes_eval(bi, torch.float64, "restated")
    assert abs(float(p[0] - q[0])) <= 1e-12 * abs(float(p[0])) and float((p[1] - q[1]).abs().max()) <= 1e-9


def test_case_lists_reach_what_they_claim():
    """the host-side arithmetic of csrc/mcb.hip's chunks() on the fusion cases, the shapes of the ragged inputs, and the
    kernel forms that the ``test_lstm_*`` docstrings of tests/test_head_gpu.py name (csrc/lstm.hip's fwd_form / bwd_form)"""
    def chunks(M, C):
        RL = max(256 // (C // 4), 1)
        per = max(-(-M // 512), 16 * RL)
        per = -(-per // RL) * RL
        return -(-M // per), per, M - (-(-M // per) - 1) * per
    rows = lambda n: R.FUSION_CASES[n]["B"] * R.FUSION_CASES[n]["T"]       # noqa: E731
    assert chunks(rows("F1"), 1024) == (2, 16, 1)
    assert chunks(rows("F2"), 1024) == (64, 16, 16)
    assert chunks(rows("F3"), 1024) == (483, 17, 14) and rows("F3") > 8192
    assert chunks(rows("F4"), 260) == (2, 48, 5) and 256 // 65 == 3 and 256 % 65 != 0
    assert chunks(rows("F6"), 12) == (2, 1360, 40) and 256 // 3 == 85
    f4, f4b = R.fusion_inputs("F4"), R.fusion_inputs("F4b")
    for h in (f4.h1, f4.h2):
        assert 0 in h.tolist() and f4.D - 1 in h.tolist()
    assert set(f4b.h1.tolist()) == {f4b.D - 1}
    for name in R.LSTM_CASES:
        li = R.lstm_inputs(name)
        assert li.lens[0] == li.T and min(li.lens) == 1 and len(li.lens) == li.B
    l2 = R.lstm_inputs("L2-T3")
    assert l2.lens[:16] == [3] * 16 and l2.lens[16:] == [1] * 16
    assert torch.equal(R.lstm_inputs("L1").x, R.lstm_inputs("L1s").x)

    def forms(name, **options):
        li = R.lstm_inputs(name)
        return (R.lstm_fwd_form(li.B, li.T, li.H, li.misalign, lstm_no_persistent=int(li.no_persistent), **options),
                R.lstm_bwd_form(li.B, li.T, li.H, li.misalign, **options))
    assert forms("L1") == (("PERSISTENT", 4, (64, 1)), "FUSED") and R.lstm_inputs("L1").T == 60
    assert forms("L1s") == (("STEP", 1, (64, 1)), "FUSED") and R.lstm_inputs("L1s").no_persistent
    assert forms("L1-T5") == (("PERSISTENT", 4, (64, 1)), "FUSED")
    assert forms("L2-T2") == forms("L2-T3") == (("PERSISTENT", 4, (64, 1)), "FUSED")
    assert forms("L3") == (("GEMM", 0, None), "FUSED") and R.lstm_inputs("L3").B == 48
    assert forms("L3p") == (("PERSISTENT", 8, (128, 1)), "FUSED")
    assert forms("L4") == (("PERSISTENT", 16, (256, 1)), "FUSED")               # exactly the 256 flags one poll covers
    assert forms("L5") == (("STEP", 4, (4, 2)), "FUSED") and R.lstm_inputs("L5").B > 64 >= R.lstm_inputs("L5").H
    assert forms("L6") == (("GEMM", 0, None), "FUSED")
    assert forms("L7") == (("GEMM", 0, None), "PLAIN")
    for name in ("L8-B16", "L8-B3"):                                             # T = 1: step 0 alone, no recurrent kernel
        assert R.lstm_inputs(name).T == 1 and forms(name)[0][0] != "PERSISTENT"
    l9 = R.lstm_inputs("L9")
    assert forms("L9") == (("GEMM", 0, None), "PLAIN") and l9.misalign
    assert (R.lstm_fwd_form(l9.B, l9.T, l9.H), R.lstm_bwd_form(l9.B, l9.T, l9.H)) == (("PERSISTENT", 4, (64, 1)), "FUSED")
    assert {n.split("-")[0] for n in R.LSTM_CASES} == {"L%d" % i for i in range(1, 10)} | {"L1s", "L3p"}
    for name in ("L1", "L5"):                                                    # what lstm_no_fused_step = 1 selects
        assert forms(name, lstm_no_fused_step=1) == (("GEMM", 0, None), "PLAIN")
    m1 = R.masked_bce_inputs("M1")
    assert sorted(set(m1.lens)) == list(range(1, 61)) and m1.logits.numel() == 15360
    assert float(R.masked_bce_inputs("Msat").logits.abs().max()) > 39


# ------------------------------------------------------------------------------------------ the bounds hold for the float32 CPU oracle
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", list(R.FUSION_CASES))
def test_fusion_bounds_hold_for_the_fp32_oracle(name, training):
    R.check_fusion(R.fusion_fp32, name, training, tag=TAG)


@pytest.mark.parametrize("name", list(R.POOLING_CASES))
def test_pooling_bounds_hold_for_the_fp32_oracle(name):
    R.check_pooling(R.pooling_fp32, name, tag=TAG)


@pytest.mark.parametrize("name", list(R.LSTM_CASES))
def test_lstm_bounds_hold_for_the_fp32_oracle(name):
    R.check_lstm(R.lstm_fp32, name, tag=TAG)


@pytest.mark.parametrize("subset", list(R.LSTM_SUBSETS))
@pytest.mark.parametrize("name", ["L6", "L1-T5"])
def test_lstm_parameter_subsets_hold_for_the_fp32_oracle(name, subset):
    R.check_lstm(R.lstm_fp32, name, frozen=R.LSTM_SUBSETS[subset], tag=TAG)


@pytest.mark.parametrize("name", list(R.MASKED_BCE_CASES))
def test_masked_bce_bounds_hold_for_the_fp32_oracle(name):
    R.check_masked_bce(R.masked_bce_fp32, name, tag=TAG)


def test_bce_2classes_bounds_hold_for_the_fp32_oracle():
    R.check_bce_2classes(R.bce_2classes_fp32, tag=TAG)


def test_worst_ratios_of_the_fp32_oracle_go_to_the_log():
    R.log_worst(TAG)


# ------------------------------------------------------------------------------------------ the assertions can fail
FUSION_MUTANTS = {            # mutant -> (case, mode) that must reject it
    "circular_off_by_one": [("F4", True), ("F5", False), ("F1", True)],
    "bn_drops_last_row": [("F5", True), ("F1", True)],
    "biased_running_var": [("F5", True), ("F2", True)],
    "row_norm": [("F4", True), ("F6", False)],
    "ssqrt_grad_at_zero": [("F5", True), ("F4", False)],
}


@pytest.mark.parametrize("mutant", list(FUSION_MUTANTS))
def test_fusion_mutants_are_rejected(mutant):
    for name, training in FUSION_MUTANTS[mutant]:
        with pytest.raises(AssertionError):
            R.check_fusion(lambda inp, tr: R.fusion_fp32(inp, tr, mutant), name, training, tag=None)
    # ... and the unmutated restatement passes where the mutant fails
    name, training = FUSION_MUTANTS[mutant][0]
    R.check_fusion(lambda inp, tr: R.fusion_fp32(inp, tr, "restated"), name, training, tag=None)


def test_pooling_mutant_is_rejected():
    with pytest.raises(AssertionError):
        R.check_pooling(lambda inp: R.pooling_fp32(inp, "circular_off_by_one"), "P1000", tag=None)


@pytest.mark.parametrize("mutant,cases", [("state_runs_on", ["L6", "L2-T3"]), ("dh_last_unit", ["L6", "L1-T5"]),
                                          ("forget_grad_c", ["L6", "L1-T5"])])
def test_lstm_mutants_are_rejected(mutant, cases):
    for name in cases:
        with pytest.raises(AssertionError):
            R.check_lstm(lambda inp, frozen: R.lstm_fp32(inp, frozen, mutant), name, tag=None)
    R.check_lstm(lambda inp, frozen: R.lstm_fp32(inp, frozen, "restated"), cases[0], tag=None)


@pytest.mark.parametrize("mutant,cases", [("norm_by_T", ["M1", "M2"]), ("first_1024_only", ["M1", "M2", "M3", "Msat"])])
def test_masked_bce_mutants_are_rejected(mutant, cases):
    for name in cases:
        with pytest.raises(AssertionError):
            R.check_masked_bce(lambda inp: R.masked_bce_fp32(inp, mutant), name, tag=None)
    R.check_masked_bce(lambda inp: R.masked_bce_fp32(inp, "restated"), cases[0], tag=None)


def test_bce_2classes_mutant_is_rejected():
    with pytest.raises(AssertionError):
        R.check_bce_2classes(lambda inp: R.bce_2classes_fp32(inp, "first_1024_only"), tag=None)
    R.check_bce_2classes(lambda inp: R.bce_2classes_fp32(inp, "restated"), tag=None)


def test_a_gradient_given_for_a_frozen_parameter_is_rejected():
    def impl(inp, frozen):
        return R.lstm_fp32(inp, ())               # ignores what is frozen
    with pytest.raises(AssertionError, match="frozen"):
        R.check_lstm(impl, "L6", frozen=("bias_ih",), tag=None)


# ------------------------------------------------------------------------------------------ host validation of the hashes
def test_count_sketch_validates_its_hashes_on_the_host():
    """``h`` indexes global memory (count_sketch_bwd_kernel) and LDS (mcb_bwd_kernel) unchecked on the device, and it is a
    registered buffer: a checkpoint can carry any value.  It is validated where the module receives it -- the constructor and
    load_state_dict -- never in forward.  No GPU test hands an out-of-range hash to a kernel."""
    from avvad import AvvadError
    from packages.models.compact_bilinear_pooling import CompactBilinearPooling, CountSketch
    ok = torch.tensor([0, 9, 3, 9, 5])
    s = torch.ones(5)
    m = CountSketch(5, 10, ok, s)
    assert torch.equal(m.h, ok)
    CountSketch(5, 10)                                                        # its own random hashes are valid
    bad = {"value = output_size": torch.tensor([0, 10, 3, 9, 5]), "negative": torch.tensor([0, -1, 3, 9, 5]),
           "int32": ok.to(torch.int32), "float": ok.float(), "too short": ok[:4], "too long": torch.cat([ok, ok]),
           "2-D": ok.view(1, 5), "huge": torch.tensor([0, 1 << 40, 3, 9, 5])}
    for what, h in bad.items():
        with pytest.raises(AvvadError):
            CountSketch(5, 10, h, s)
        sd = {"h": h, "s": s}
        with pytest.raises(AvvadError):
            m.load_state_dict(sd)
        assert torch.equal(m.h, ok), what                                     # a refused load leaves the module as it was
    with pytest.raises(AvvadError):
        CountSketch(5, 10, [0, 1, 2, 3, 4], s)                                # not a tensor
    m.load_state_dict({"h": torch.tensor([9, 9, 9, 9, 0]), "s": -s})
    assert m.h.tolist() == [9, 9, 9, 9, 0]
    pool = CompactBilinearPooling(5, 4, 10, ok, s, torch.tensor([1, 2, 3, 4]), torch.ones(4))
    sd = {k: t.clone() for k, t in pool.state_dict().items()}
    assert sorted(sd) == ["sketch1.h", "sketch1.s", "sketch2.h", "sketch2.s"]
    pool.load_state_dict(sd)
    sd["sketch2.h"][2] = 10
    with pytest.raises(AvvadError, match="sketch2"):
        pool.load_state_dict(sd)
    with pytest.raises(AvvadError):
        CompactBilinearPooling(5, 4, 10, ok, s, torch.tensor([1, 2, 3, 10]), torch.ones(4))
    # the module keeps h int64 through a dtype cast, and forward validates nothing (it only refuses host tensors)
    assert m.double().h.dtype == torch.long
    with pytest.raises(AvvadError, match="GPU"):
        m.float()(torch.zeros(2, 5))
