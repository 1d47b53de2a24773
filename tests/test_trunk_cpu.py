"""CPU tests of the whole-trunk oracle (tests/trunk_ref.py): the restatement against ``oracle.resnet18``, the TAU table against
the measured float32 spread, the cap on differing decisions, every case and gradient subset of tests/test_trunk_gpu.py with the
float32 CPU evaluation in the place of the HIP path (the bounds are within reach of a correct float32 evaluation, and the
harness works), the case and variant tables against the restated form choices of csrc/trunk.hip, and mutants of the stand-in
that ``check_trunk`` must reject."""
import pytest
import torch

import trunk_ref as R
from oracle import resnet18


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("case", ["T7", "T7e"])
def test_restatement_is_the_oracle_in_float64(case):
    """features, all 60 gradients (20 convolutions, 20 x 2 BatchNorm) and the 40 running statistics of
    ``oracle.resnet18.trunk_forward`` (three equal input channels, F.batch_norm, F.relu, F.max_pool2d) to float64 rounding"""
    inp, ref = R.inputs(case), R.reference(case)
    sd = {"features." + k: (v.double().clone() if v.is_floating_point() else v.clone()) for k, v in inp.sd.items()}
    for k in R.param_keys():
        sd["features." + k].requires_grad_(True)
    out, inter = resnet18.trunk_forward(sd, inp.x.double()[:, None].repeat(1, 3, 1, 1), inp.training, return_intermediates=True)
    (out * inp.G.double()).sum().backward()
    assert float((out.detach() - ref.feat).abs().max()) <= 1e-12 * max(1.0, float(ref.feat.abs().max()))
    for k in R.param_keys():
        g = sd["features." + k].grad
        assert float((g - ref.grads[k]).abs().max()) <= 1e-11 * max(1.0, float(g.abs().max())), k
    for k, v in ref.stats.items():
        assert float((sd["features." + k] - v).abs().max()) <= 1e-13, k
    inter = {k: v.detach() for k, v in inter.items()}
    for k in R.NAMES:                                # and the 17 layers are the oracle's
        assert torch.equal(inter[k] > 0, ref.masks[k]), k
        assert float((inter[k] - ref.pre[k].clamp(min=0)).abs().max()) <= 1e-11 * max(1.0, float(inter[k].max())), k
    assert len(R.param_keys()) == 60 and len(ref.stats) == 40 and len(ref.pre) == 17


def test_pool_positions_are_the_first_maximum_in_scan_order():
    """exact ties (a flat frame region): position of the first maximum, torch's max_pool2d rule, and the window cut short
    on an odd grid"""
    z = torch.zeros(1, 1, 5, 4, dtype=torch.float64)
    z[0, 0, 1:3, 1:3] = 2.0
    z[0, 0, 4, 3] = 1.0
    yw = R.pool_windows(z, float("-inf"))
    am = yw.argmax(0)
    _, idx = torch.nn.functional.max_pool2d(z, 3, 2, 1, return_indices=True)
    h = 2 * torch.arange(3)[:, None] - 1 + am[0, 0] // 3
    w = 2 * torch.arange(2)[None, :] - 1 + am[0, 0] % 3
    assert torch.equal(h * 4 + w, idx[0, 0])
    assert torch.isinf(yw[:, 0, 0, 2, :][6:]).all()            # the third row of the last windows is outside the 5-row grid


# ------------------------------------------------------------------------------------------ TAU and the cap
def spreads(case):
    """per layer: max |pre32 - pre64| of the float32 CPU evaluation; the oracle's own float32 post-ReLU values against
    relu(pre64) (the same quantity where the oracle states it); and the decisions that differ"""
    ref, r32 = R.reference(case), R.run(case, torch.float32)
    inp = R.inputs(case)
    sd = {"features." + k: v.clone() for k, v in inp.sd.items()}
    with torch.no_grad():
        _, inter = resnet18.trunk_forward(sd, inp.x[:, None].repeat(1, 3, 1, 1), inp.training, return_intermediates=True)
    sp = []
    for k in R.NAMES:
        a = float((r32.pre[k].double() - ref.pre[k]).abs().max())
        b = float((inter[k].double() - ref.pre[k].clamp(min=0)).abs().max())
        sp.append(max(a, b))
    got = dict(masks=r32.masks, argmax=r32.argmax)
    n_relu, n_pool, bad = R.decisions(got, ref, case)
    return sp, n_relu, n_pool, bad


@pytest.mark.parametrize("case", list(R.CASES))
def test_tau_table_and_cap(case):
    """TAU[case][k] is 8 .. 16 x the float32 spread of layer k (recorded at 10 x), and the float32 evaluation's own
    differing decisions are inside the rule and within the cap"""
    sp, n_relu, n_pool, bad = spreads(case)
    print("%-4s spread %s" % (case, " ".join("%.2e" % s for s in sp)))
    print("%-4s decisions that differ from float64: %d ReLU + %d pool of %d units, cap %d" % (case, n_relu, n_pool, R.units(case), R.cap(case)))
    for k, s, t in zip(R.NAMES, sp, R.TAU[case]):
        assert 8.0 * s <= t <= 16.0 * s, (case, k, s, t)
    assert not bad, bad
    assert n_relu + n_pool <= R.cap(case)
    assert R.units(case) == sum(v.numel() for v in R.reference(case).pre.values())


# ------------------------------------------------------------------------------------------ the float32 evaluation under the checks
@pytest.mark.parametrize("case", list(R.CASES))
def test_float32_evaluation_passes(case):
    R.check_trunk(R.trunk_fp32, case, tag="cpu")


@pytest.mark.parametrize("case", ["T7", "T1"])
@pytest.mark.parametrize("subset", list(R.SUBSETS))
def test_float32_evaluation_passes_subsets(case, subset):
    frozen = R.frozen_keys(subset)
    assert 0 < len(frozen) < 60
    R.check_trunk(lambda inp, fr: R.trunk_fp32(inp, fr), case, frozen=frozen, tag="cpu")


@pytest.mark.parametrize("case", ["T7", "T1"])
def test_float32_evaluation_passes_accumulate(case):
    R.check_trunk(lambda inp, fr: R.trunk_fp32(inp, fr, accumulate=True), case, accumulate=True, tag="cpu")
    R.log_worst("cpu")


def test_subsets_name_what_they_claim():
    keys = R.param_keys()
    assert R.frozen_keys("stem_frozen") == ("0.weight", "1.weight", "1.bias")
    assert len(R.frozen_keys("convs_frozen")) == 20 and len(R.frozen_keys("bn_frozen")) == 40
    assert [k for k in keys if k not in R.frozen_keys("only_7_1")] == ["7.1.conv1.weight", "7.1.bn1.weight", "7.1.bn1.bias",
                                                                        "7.1.conv2.weight", "7.1.bn2.weight", "7.1.bn2.bias"]


# ------------------------------------------------------------------------------------------ what the cases reach
def _chain(case):
    c = R.CASES[case]
    g = R.geoms(c["N"], c["H"], c["W"])
    return [(g[0].Ho, g[0].Wo)] + [(g[i].Ho, g[i].Wo) for i in (1, 5, 10, 15)]


def test_cases_reach_what_they_claim():
    f = {case: R.forms(case) for case in R.CASES}
    assert _chain("T1") == [(18, 22), (9, 11), (5, 6), (3, 3), (2, 2)] == _chain("T3")
    assert _chain("T2") == [(26, 18), (13, 9), (7, 5), (4, 3), (2, 2)]
    assert _chain("T4") == [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    assert _chain("T5") == [(18, 38), (9, 19), (5, 10), (3, 5), (2, 3)]
    assert _chain("T6") == [(18, 18), (9, 9), (5, 5), (3, 3), (2, 2)]
    assert _chain("T7") == [(17, 20), (9, 10), (5, 5), (3, 3), (2, 2)]
    assert _chain("T8") == [(34, 34), (17, 17), (9, 9), (5, 5), (3, 3)]
    # T1: every form in one trunk; one convolution with three different ones; ragged class tiles feed fused statistics
    assert f["T1"]["0"] == ("STEM", None, "STEM", 130)
    assert f["T1"]["4.0.conv1"] == ("CONV64", "CONV64", "CONV64", 256)
    assert f["T1"]["5.0.conv1"] == ("CLS", "PARITY 128x64 buf", "ENGINE 128x128 buf", 5 * 6 * 2)
    assert f["T1"]["5.0.conv2"] == ("CLS", "CLS", "TAP", 60)
    assert f["T1"]["5.0.downsample.0"][0].startswith("ENGINE") and f["T1"]["5.0.downsample.0"][1].startswith("PARITY")
    assert f["T1"]["6.0.conv1"] == ("CLS", "CLS", "TAP", 18)          # the stride-2 data gradient as one class product, 6 -> 3
    assert R.geoms(130, 35, 43)[10].W == 6 and R.geoms(130, 35, 43)[10].Wo == 3
    assert f["T1"]["7.1.conv2"] == ("CLS", "CLS", "TAP", 8)
    assert all(r[3] is None for r in f["T1e"].values()) and [r[:3] for r in f["T1e"].values()] == [r[:3] for r in f["T1"].values()]
    # T2: whole class tiles, an even 4 -> 2 step as a class product
    assert f["T2"]["7.0.conv1"][:3] == ("CLS", "CLS", "TAP") and R.geoms(128, 51, 35)[15].H == 4
    assert f["T2"]["5.0.conv2"] == ("CLS", "CLS", "TAP", 35)
    # T3: no class form anywhere
    assert not any(x in ("CLS", "TAP") for r in f["T3"].values() for x in r[:3])
    assert f["T3"]["5.0.conv1"][:3] == ("ENGINE 128x128 buf", "PARITY 128x64 buf", "ENGINE 128x128 buf")
    # T4: the 1x1 last stage is refused beside classes in layers 2 and 3
    assert all(f["T4"][k][0] == "CLS" for k in ("5.0.conv1", "5.1.conv2", "6.0.conv1", "6.1.conv2"))
    assert all(f["T4"][k][0].startswith("ENGINE") and f["T4"][k][2].startswith("ENGINE") for k in ("7.0.conv1", "7.0.conv2", "7.1.conv1", "7.1.conv2"))
    assert f["T4"]["7.0.conv1"][1].startswith("PARITY") and f["T4"]["7.1.conv1"][1].startswith("ENGINE")
    # T5: stem and conv64 forward on their kernels, both weight gradients on the engine
    assert f["T5"]["0"] == ("STEM", None, "ENGINE 64x64", 129)
    assert f["T5"]["4.1.conv2"][:3] == ("CONV64", "CONV64", "ENGINE 128x64 buf")
    assert f["T1"]["4.1.conv2"][2] == "CONV64" and f["T1"]["0"][2] == "STEM"
    # T6: three class-row tiles, the stem backward's grid at its cap
    assert f["T6"]["6.1.conv1"] == ("CLS", "CLS", "TAP", 27) and R.stem_bwd_grid("T6") == 2048 < R.stem_bwd_grid("T6", no_fused_stats=1)
    assert R.stem_bwd_grid("T7") == 128
    # T7: the small-N forms on an odd stem grid
    assert f["T7"]["0"][0] == "STEM" and f["T7"]["0"][2] == "STEM" and _chain("T7")[0][0] % 2 == 1
    assert f["T7"]["5.0.conv1"][:3] == ("ENGINE 128x128 buf", "PARITY 128x64 buf", "ENGINE 128x128 buf")
    assert f["T7"]["4.0.conv1"][:3] == ("CONV64", "CONV64", "CONV64")
    # T8: the workload's geometry: 9x9 classes at 2 row tiles
    assert f["T8"]["5.0.conv2"] == ("CLS", "CLS", "TAP", 162) and f["T8"]["7.1.conv2"] == ("CLS", "CLS", "TAP", 18)


@pytest.mark.parametrize("label,options,cases,base", R.VARIANTS, ids=[v[0] for v in R.VARIANTS])
def test_every_variant_changes_a_form(label, options, cases, base):
    for case in cases:
        assert R.forms(case, **options) != R.forms(case, **base), (label, case)
    if label == "cls_cap40":                         # 5x6 grids fall to the engine, 3x3 and 2x2 stay classes
        f = R.forms("T1", **options)
        assert f["5.0.conv2"][0].startswith("ENGINE") and f["6.0.conv2"][0] == "CLS" and f["7.0.conv2"][0] == "CLS"
    if label == "bwd_max_cus8":                      # the backward takes other forms than the forward did
        f = R.forms("T1", **options)
        assert f["5.0.conv2"] == ("CLS", "ENGINE 128x128 buf", "TAP", 60) and f["7.0.conv2"][1] == "CLS"
    assert R.forms("T1", no_fixup1=1) == R.forms("T1")          # (why no_fixup1 is no variant: it changes no form)


# ------------------------------------------------------------------------------------------ mutants
def _rejected(impl, case, **kw):
    with pytest.raises(AssertionError):
        R.check_trunk(impl, case, tag=None, **kw)


@pytest.mark.parametrize("mutant,case", [
    ("pool_second_best", "T7"), ("pool_hw_swapped", "T1"), ("pool_hw_swapped", "T2"), ("pool_drops_last", "T7"),
    ("stats_skip_rows_128", "T1"), ("stats_count_padded", "T1"), ("bn_bwd_no_mean_term", "T7"), ("running_var_biased", "T7"),
    ("a1_mask_from_output", "T7"), ("identity_before_ds_bn", "T7"), ("s2_dgrad_misses_last", "T1"),
    ("s2_dgrad_misses_last", "T2"), ("wgrad_short_of_last_image", "T5"), ("wgrad_short_of_last_image", "T6")])
def test_mutant_is_rejected(mutant, case):
    _rejected(lambda inp, fr: R.trunk_fp32(inp, fr, mutant=mutant), case)


def test_pool_hw_swapped_is_invisible_on_a_square_grid():
    """(what the suite's 67x67 frames could not see)"""
    a, b = R.run("T6", torch.float32, mutant="pool_hw_swapped", keep_pre=False), R.run("T6", torch.float32, keep_pre=False)
    assert torch.equal(a.feat, b.feat)


def test_dbeta_overwritten_is_rejected():
    def impl(inp, fr):
        r = R.trunk_fp32(inp, fr, accumulate=True)
        for k in r["grads"]:
            if k.endswith(".bias"):
                r["grads"][k] = r["grads"][k] - R.prefill(k, r["grads"][k].shape)
        return r
    _rejected(impl, "T7", accumulate=True)


def test_frozen_parameter_with_a_gradient_is_rejected():
    _rejected(lambda inp, fr: R.trunk_fp32(inp, ()), "T7", frozen=R.frozen_keys("stem_frozen"))


def _pinned_with_flips(case, picks):
    """the float32 evaluation under float64's decisions with the units ``picks`` (layer, flat index) on the other side"""
    ref = R.reference(case)
    masks = {k: v.clone() for k, v in ref.masks.items()}
    for k, i in picks:
        masks[k].view(-1)[i] ^= True
    return lambda inp, fr: R.trunk_fp32(inp, fr, masks=masks, argmax=ref.argmax)


def _smallest(case, n):
    """the n units with the smallest |pre64| (layer, flat index), all of them inside the rule"""
    ref, t = R.reference(case), R.tau(case)
    cand = []
    for k in R.NAMES:
        a = ref.pre[k].abs().reshape(-1)
        v, i = a.topk(min(n, a.numel()), largest=False)
        cand += [(float(x), k, int(j)) for x, j in zip(v, i) if float(x) <= t[k]]
    cand.sort()
    assert len(cand) >= n, (case, len(cand))
    return [(k, i) for _, k, i in cand[:n]]


def test_a_flip_at_1e_3_is_rejected_and_flips_inside_the_rule_pass_up_to_the_cap():
    case = "T7"
    ref = R.reference(case)
    n = R.cap(case)
    assert R.check_trunk(_pinned_with_flips(case, _smallest(case, n)), case, tag=None) == (n, 0)      # exactly the cap: passes
    with pytest.raises(AssertionError, match="more than the cap"):
        R.check_trunk(_pinned_with_flips(case, _smallest(case, n + 1)), case, tag=None)
    a = (ref.pre["5.1.a1"].abs().reshape(-1) - 1e-3).abs()
    i = int(a.argmin())
    assert 5e-4 < abs(float(ref.pre["5.1.a1"].reshape(-1)[i])) < 2e-3
    with pytest.raises(AssertionError, match="on the other side"):
        R.check_trunk(_pinned_with_flips(case, [("5.1.a1", i)]), case, tag=None)


def test_a_pool_position_outside_the_rule_is_rejected():
    case = "T7"
    ref = R.reference(case)
    yw = R.pool_windows(ref.z0.clamp(min=0), float("-inf"))
    top2 = yw.topk(2, dim=0)
    gap = (top2.values[0] - top2.values[1]).reshape(-1)
    i = int(((gap - 1e-2).abs()).argmin())                      # a window whose runner-up is ~1e-2 below its maximum
    am = ref.argmax.clone()
    am.view(-1)[i] = top2.indices[1].reshape(-1)[i].to(torch.uint8)
    with pytest.raises(AssertionError, match="below float64's maximum"):
        R.check_trunk(lambda inp, fr: R.trunk_fp32(inp, fr, masks=ref.masks, argmax=am), case, tag=None)
