"""CPU tests of the bf16 trunk's value-pinned float64 replay (tests/trunk_ref.py, the bf16 section): the float64 rounding
helper, the D16 table and B16 against what the float32 stand-in measures, the two-value share of the forward rule on the
float64 reference's own values, every case of tests/test_trunk_bf16_gpu.py with the float32 stand-in in the place of the HIP
path, the bf16 form choices of csrc/trunk.hip restated and what each case reaches, and mutants of the stand-in that
``check_trunk_bf16`` must reject -- each by the check that is there to catch it."""
import functools

import pytest
import torch

import trunk_ref as R


# ------------------------------------------------------------------------------------------ the rounding helper
def test_rne_bf16_in_float64_is_one_rounding():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(200000, generator=g) * torch.exp2(torch.randint(-20, 20, (200000,), generator=g).float())
    assert torch.equal(R.rne_bf16(x.double()), x.bfloat16().double())          # float32 values: torch's own rounding
    assert torch.equal(R.rne_bf16(x), x.bfloat16().float())
    one, ulp = 1.0, 2.0 ** -7
    t = torch.tensor([one + ulp / 2, one + 3 * ulp / 2, one + ulp / 2 + 1e-12, one + ulp / 2 - 1e-12, -(one + ulp / 2 + 1e-12), 0.0],
                     dtype=torch.float64)
    assert R.rne_bf16(t).tolist() == [one, one + 2 * ulp, one + ulp, one, -(one + ulp), 0.0]      # ties to even; no float32 step
    assert float(torch.tensor([one + ulp / 2 + 1e-12]).double()) != one + ulp / 2 + 1e-12           # (float32 would have lost it)
    assert R.trunc_bf16(t).tolist() == [one, one + ulp, one, one, -one, 0.0]
    assert torch.equal(R.trunc_bf16(x).double(), R.trunc_bf16(x.double()))


# ------------------------------------------------------------------------------------------ D16, B16, the two-value share
@functools.lru_cache(maxsize=None)
def measured(case):
    """-> (per entry of D_NAMES: max |v32 - v64| of the float32 stand-in under the same pinning; its worst gradient distance
    / max(1, max|ref|) and that gradient's name)"""
    got = R.trunk_bf16_standin(R.inputs(case))
    ref = R.replay(case, got)             # (pinned to the stand-in's own stored values: the stand-in IS the float32 evaluation under that pinning)
    sp = [float((got["z0"].double() - ref.z0).abs().max())] + [float((got["v"][k].double() - ref.v[k]).abs().max()) for k in R.NAMES]
    worst = max((float((got["grads"][k].double() - ref.grads[k]).abs().max()) / max(1.0, float(ref.grads[k].abs().max())), k)
                for k in R.param_keys())
    return tuple(sp), worst


@pytest.mark.parametrize("case", list(R.CASES))
def test_d16_table_and_two_value_share(case):
    """D16[case][k] is 8 .. 16 x the float32 spread of layer k under the pinning (recorded at 10 x), and on the float64
    reference's own values at most 5 % of a layer's elements have a two-value admissible set"""
    sp, (e, k) = measured(case)
    print("%-4s spread %s" % (case, " ".join("%.2e" % s for s in sp)))
    print("%-4s worst float32 gradient distance %.3e (%s)" % (case, e, k))
    for name, s, d in zip(R.D_NAMES, sp, R.D16[case]):
        assert 8.0 * s <= d <= 16.0 * s, (case, name, s, d)
    own = R.run16(case, torch.float64)
    shares = R.two_value_shares(own.v, case)
    print("%-4s two-value share %s" % (case, " ".join("%.4f" % s for s in shares)))
    assert max(shares) <= R.TWO_VALUE_CAP, (case, shares)


def test_b16_is_10x_the_float32_distance():
    e = max(measured(case)[1] for case in R.CASES)
    print("E32 measured %.4e (%s), recorded %.4e, B16 %.3e" % (e[0], e[1], R.E32, R.B16))
    assert R.B16 == max(1e-4, 10 * R.E32)
    assert 8.0 * e[0] <= R.B16 <= 16.0 * e[0] or (R.B16 == 1e-4 and 8.0 * e[0] <= 1e-4)


# ------------------------------------------------------------------------------------------ the stand-in under the checks
@pytest.mark.parametrize("case", list(R.CASES))
def test_standin_passes(case):
    R.check_trunk_bf16(R.trunk_bf16_standin, case, tag="cpu")


def test_standin_passes_stem_frozen_and_accumulate():
    frozen = R.frozen_keys("stem_frozen")
    R.check_trunk_bf16(lambda inp, fr: R.trunk_bf16_standin(inp, fr), "T1", frozen=frozen, options_label="stem_frozen", tag="cpu")
    R.check_trunk_bf16(lambda inp, fr: R.trunk_bf16_standin(inp, fr, accumulate=True), "T7", accumulate=True, tag="cpu")
    R.log_worst16("cpu")


# ------------------------------------------------------------------------------------------ what the cases reach
def test_bf16_forms_of_the_cases():
    f = {case: R.forms16(case) for case in R.CASES}
    eng, par = "ENGINE 128x128 buf", "PARITY 128x128 buf"
    for case in R.CASES:                             # conv64::kernel<B16, .> in layer 1 everywhere; its weight gradient on the engine
        assert all(f[case]["4.%d.conv%d" % (b, j)][:3] == ("CONV64", "CONV64", "ENGINE 128x64 buf") for b in (0, 1) for j in (1, 2))
        assert f[case]["0"] == R.forms(case)["0"]
    # T1, T8: CLS16 forward on 3x3 and 2x2 grids, two row tiles, the second ragged, feeding the fused statistics
    assert f["T1"]["6.1.conv2"] == ("CLS", "CLS", "TAP", 3 * 3 * 2) and f["T1"]["7.1.conv2"] == ("CLS", "CLS", "TAP", 2 * 2 * 2)
    assert f["T8"]["7.1.conv2"] == ("CLS", "CLS", "TAP", 18) and R.CASES["T1"]["N"] % 128 and R.CASES["T8"]["N"] % 128
    # ... and refused on 5x6 / 5x5 and larger grids, on 1x1, and one frame below the threshold
    assert f["T1"]["5.1.conv2"] == (eng, eng, eng, 31) and f["T8"]["6.1.conv2"] == (eng, eng, eng, 26)
    assert f["T4"]["7.1.conv2"] == (eng, eng, eng, 2) and f["T4"]["6.1.conv2"][:3] == ("CLS", "CLS", "TAP")
    assert not any(x in ("CLS", "TAP") for r in f["T3"].values() for x in r[:3])
    assert f["T2"]["6.1.conv2"][0] == eng and f["T2"]["7.1.conv2"][:3] == ("CLS", "CLS", "TAP")          # 4x3 = 12 > 9
    # the stride-2 data gradient: one class product at C >= 128 on every grid, PARITY at C = 64 and for the 1x1 downsample
    for case in ("T1", "T2", "T5", "T8"):
        assert f[case]["6.0.conv1"][1] == "CLS" and f[case]["5.0.conv1"][1] == "PARITY 128x64 buf"
        assert f[case]["6.0.downsample.0"][1] == par
    assert f["T8"]["6.0.conv1"] == (eng, "CLS", eng, 26) and f["T3"]["6.0.conv1"][1] == par and f["T7"]["6.0.conv1"][1] == par
    # TAP16 beside the engine for the weight gradient
    assert f["T1"]["6.0.conv1"][2] == "TAP" and f["T1"]["5.0.conv2"][2] == eng and f["T1"]["6.0.downsample.0"][2] == eng
    # eval mode: the same forms, no statistics; small N: no class anywhere; three row tiles
    assert all(r[3] is None for r in f["T1e"].values()) and [r[:3] for r in f["T1e"].values()] == [r[:3] for r in f["T1"].values()]
    assert all(r[3] is None for r in f["T7e"].values())
    assert not any(x in ("CLS", "TAP") for r in f["T7"].values() for x in r[:3]) and f["T7"]["4.0.conv1"][3] == 17
    assert f["T6"]["6.1.conv1"] == ("CLS", "CLS", "TAP", 27) and f["T6"]["7.1.conv1"] == ("CLS", "CLS", "TAP", 12)
    # the stem: LDS kernels exact; T5's weight gradient on the engine, whose staging rounds both operands
    assert R.stem_rounding("T5") == {"wgrad"} and f["T5"]["0"] == ("STEM", None, "ENGINE 64x64", 129)
    assert all(R.stem_rounding(case) == set() for case in R.CASES if case != "T5")
    assert R.stem_rounding("T7", no_stem_kernel=1) == {"fwd", "wgrad"}


@pytest.mark.parametrize("label,options,cases", R.VARIANTS16, ids=[v[0] for v in R.VARIANTS16])
def test_every_bf16_variant_changes_a_form(label, options, cases):
    for case in cases:
        a, b = R.forms16(case), R.forms16(case, **options)
        assert any(a[k] != b[k] for k in a if k != "0"), (label, case)
    if label == "bwd_max_cus8":                      # the backward takes other forms than the forward did
        assert R.forms16("T1", **options)["6.1.conv1"] == ("CLS", "ENGINE 128x128 buf", "ENGINE 128x128 buf", 18)
    if label == "no_s2_cls":
        assert R.forms16("T1", **options)["6.0.conv1"] == ("CLS", "PARITY 128x128 buf", "TAP", 18)


# ------------------------------------------------------------------------------------------ mutants
MUTANT_RUNS = [
    ("store_truncates", "T7", "rule: "), ("bn2_rounded_before_add", "T7", "rule: "), ("ds_identity_rounded", "T7", "rule: "),
    ("input_fp32_pitch", "T7", "rule: 5.1"), ("mask_bits_reversed", "T7", "gradient: "), ("mask_shifted_quad", "T7", "gradient: "),
    ("stats_skip_rows_128", "T1", "running statistics: "), ("stem_rounds_operands", "T7", "rule: pool"),
]


@pytest.mark.parametrize("mutant,case,caught_by", MUTANT_RUNS, ids=[m[0] for m in MUTANT_RUNS])
def test_mutant_is_rejected(mutant, case, caught_by):
    with pytest.raises(AssertionError) as e:
        R.check_trunk_bf16(lambda inp, fr: R.trunk_bf16_standin(inp, fr, mutant=mutant), case, tag=None)
    assert "\n" + caught_by in str(e.value), str(e.value)[:2000]


def test_mask_mutants_leave_the_forward_alone():
    """(the byte mask's mutants are wrong in the backward only: nothing but the gradients can see them)"""
    for mutant in ("mask_bits_reversed", "mask_shifted_quad"):
        with pytest.raises(AssertionError) as e:
            R.check_trunk_bf16(lambda inp, fr: R.trunk_bf16_standin(inp, fr, mutant=mutant), "T7", tag=None)
        assert "\nrule: " not in str(e.value) and "\nrunning statistics: " not in str(e.value) and "\nfeatures: " not in str(e.value)


def test_stem_engine_rounding_is_restated():
    """T5's stem weight gradient runs on the engine, whose staging rounds x and d c0 to bf16: the replay restates it (only
    d/d 0.weight moves, by 2.4e-3 of its maximum).  The gradient bound B16 cannot see a fault of that size: see below."""
    a, b = R.run16("T5", torch.float64, stem=frozenset({"wgrad"})), R.run16("T5", torch.float64, stem=frozenset())
    moved = [k for k in R.param_keys() if not torch.equal(a.grads[k], b.grads[k])]
    assert moved == ["0.weight"]
    rel = float((a.grads["0.weight"] - b.grads["0.weight"]).abs().max() / b.grads["0.weight"].abs().max())
    print("T5 d/d 0.weight: engine rounding moves it by %.2e of its maximum" % rel)
    assert 5e-4 < rel < 1e-2
    assert torch.equal(a.feat, b.feat) and all(torch.equal(a.acts[k], b.acts[k]) for k in R.NAMES)


@pytest.mark.parametrize("mutant", ["dgrad_pack_via_fp16", "dgrad_weights_unrounded"])
def test_weight_mutants_of_the_data_gradient_are_not_told_from_a_valid_evaluation(mutant):
    """DROPPED as rejected mutants, and why: a data gradient that multiplies weights rounded through fp16 first, or not rounded
    at all, is a 2^-9 relative change of the weights.  The backward's bf16 cotangent stores are not pinned (the stored
    cotangents are overwritten before they can be read), so a cotangent that float32 noise puts on the other bf16 neighbour
    moves the next layer's cotangents across their boundaries too, and 4 .. 5 layers below the last block a VALID float32
    evaluation is already 0.9 .. 1.1e-2 max(1, max|ref|) from the float64 replay (E32).  These mutants are at 1.3 .. 1.5e-2:
    inside what a valid evaluation does, far inside B16.  The forward and the statistics do not see them at all."""
    got = R.trunk_bf16_standin(R.inputs("T7"), mutant=mutant)
    ref = R.replay("T7", got)
    w = max(float((got["grads"][k].double() - ref.grads[k]).abs().max()) / max(1.0, float(ref.grads[k].abs().max())) for k in R.param_keys())
    print("%s: worst gradient distance %.3e, E32 %.1e, B16 %.2e" % (mutant, w, R.E32, R.B16))
    assert w < 3 * R.E32 < R.B16
    R.check_trunk_bf16(lambda inp, fr: got, "T7", tag=None)


def test_a_far_neighbour_at_100_d_from_the_boundary_is_rejected():
    case, k = "T7", "6.0"
    got = R.trunk_bf16_standin(R.inputs(case))
    ref = R.replay(case, got)
    v, s, d = ref.v[k], got["acts"][k].double(), R.d16(case)[k]
    up = R.rne_bf16(s * (1 + 2.0 ** -7))                                    # the bf16 neighbour above (s > 0)
    dist = ((s + up) / 2 - v).abs()                                          # |v - boundary|
    pick = (s > 0.5) & (s == R.rne_bf16(v.clamp(min=0)))
    i = int(torch.where(pick, (dist - 100 * d).abs(), torch.full_like(dist, 1e9)).reshape(-1).argmin())
    assert 50 * d < float(dist.reshape(-1)[i]) < 200 * d
    acts = dict(got["acts"])
    acts[k] = got["acts"][k].clone()
    acts[k].view(-1)[i] = float(up.reshape(-1)[i])
    idx = tuple(int(j) for j in torch.unravel_index(torch.tensor(i), s.shape))
    with pytest.raises(AssertionError) as e:
        R.check_trunk_bf16(lambda inp, fr: dict(got, acts=acts), case, tag=None)
    assert "\nrule: %s%s stored" % (k, idx) in str(e.value), str(e.value)[:1500]


def test_a_float32_view_of_the_bf16_bytes_is_rejected():
    """what ``ops.trunk_saved_activations`` returned under option bf16 before it decoded the storage"""
    got = R.trunk_bf16_standin(R.inputs("T7"))
    acts = dict(got["acts"])
    a = got["acts"]["pool"].permute(0, 2, 3, 1).contiguous().bfloat16()
    raw = torch.cat([a.reshape(-1), a.reshape(-1)]).view(torch.float32)      # bf16 bytes read as float32
    acts["pool"] = raw.reshape(a.shape).permute(0, 3, 1, 2).nan_to_num(0.0).abs()
    with pytest.raises(AssertionError, match="no bf16 values"):
        R.check_trunk_bf16(lambda inp, fr: dict(got, acts=acts), "T7", tag=None)
