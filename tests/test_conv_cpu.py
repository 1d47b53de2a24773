"""CPU tests of the single-convolution oracle (tests/conv_ref.py): the restated kernel-form choice against the source text
and against what every case claims to reach, every case of tests/test_conv_gpu.py with a float32 im2col evaluation in the
place of the HIP path (the rounding bound is within reach of correct float32 arithmetic), and mutants of that evaluation
which ``check_conv`` must reject."""
import inspect
import os
import re

import numpy as np
import pytest

import conv_ref as R

TAG = "cpu32"


def _src(name):
    with open(os.path.join(R.CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------ the restatement against the source
def test_constants_match_the_source():
    """the constants conv_plan aims the cases with, read back from the source text: a change there fails here"""
    trunk, conv64 = _src("trunk.hip"), _src("conv64.h")
    assert int(re.search(r"constexpr int WG_MAXW = (\d+);", conv64).group(1)) == R.WG_MAXW
    m = re.search(r"constexpr int WROWS = (\d+) \* (\d+);", conv64)
    assert int(m.group(1)) * int(m.group(2)) * 64 == R.WG_PART and "WG_PART = WROWS * 64;" in conv64
    assert int(re.search(r"constexpr int STEM_WH = (\d+);", trunk).group(1)) == R.STEM_WH
    m = re.search(r"\(size_t\)\(g\.H \+ 6\) \* LDW \* sizeof\(float\) <= (\d+) \* 1024", trunk)
    assert int(m.group(1)) * 1024 == R.STEM_LDS and "const int LDW = (g.W + 6) | 1;" in trunk
    assert int(re.search(r"return (\d+)L \* grid_cus\(\);", trunk).group(1)) == R.CLS_TILES_PER_CU
    assert "n_floats < (1L << 29) - 64" in trunk and R.FITS_BUF == (1 << 29) - 64
    assert "n < (1L << 30)" in trunk and R.FITS_U30 == 1 << 30
    assert "return g.KS * g.KS <= 32;" in trunk
    # the tile choices and the per-CU workgroup counts engine_rounds restates
    assert "const int cols = g.Co <= 64 ? 64 : 128;" in trunk and "const int cols = g.C <= 64 ? 64 : 128;" in trunk
    assert "if (variant == 3) per_cu = 2;" in _src("igemm.h")
    assert "const long T = (M + 31) / 32;" in conv64 and "return (int)(T < cus ? (T > 0 ? T : 1) : cus);" in conv64
    # the parity classes' tap counts
    assert "c.nkh = c.kh0 < g.KS ? (g.KS - c.kh0 + 1) / 2 : 0;" in trunk and "c.kh0 = (ph + g.pad) & 1; c.kw0 = (pw + g.pad) & 1;" in trunk
    assert "__host__ __device__ static int cnt2(int h, int q) { const int m = h >> 1; return h + (m < q - 1 ? m : q - 1); }" in _src("igemm.h")


def test_cited_lines_hold():
    """every line number in conv_plan's comments still holds the text it is cited for"""
    lines = {f: _src(f).split("\n") for f in {c[0] for c in R.CITES}}
    for f, n, text in R.CITES:
        assert text in lines[f][n - 1], "%s:%d no longer holds %r: move the citation in conv_ref and in CITES" % (f, n, text)
    cited = set()
    src = "".join(inspect.getsource(f) for f in (R.conv_plan, R.geom, R._cls_tile_cap, R._stem_kernel_ok, R._stem_wgrad_ok, R._cls_common,
                                                 R._fwd_cls_ok, R._dgrad_cls_ok, R._wgrad_tap_ok, R._conv64_ok, R._conv64_wgrad_ok,
                                                 R._bf16_conv_ok, R._cls16_common, R._fwd16_cls_ok, R._dgrad16_cls_ok, R._wgrad16_tap_ok,
                                                 R._pool, R._last_cut, R.engine_rounds))
    for m in re.finditer(r"lines? (\d+)(?:-(\d+))?(?:, (\d+))?(?:, (\d+))?\)", src):
        cited.update(int(g) for g in m.groups() if g)
    assert cited and cited <= {n for _, n, _ in R.CITES}, sorted(cited - {n for _, n, _ in R.CITES})


def test_the_dgrad_parity_refusals_come_before_the_first_launch():
    """trunk.hip dgrad_parity: both AVVAD_EINVAL returns stand in front of the zero-fill of dx"""
    body = _src("trunk.hip")
    body = body[body.index("static int dgrad_parity("):body.index("// (the ENGINE and PARITY forms)")]
    zero = body.index("hipLaunchKernelGGL(zero_f32")
    refusals = [m.start() for m in re.finditer("return AVVAD_EINVAL", body)]
    assert len(refusals) == 2 and all(r < zero for r in refusals)


def test_cases_reach_what_they_claim():
    """every case against conv_plan, and what the cases must reach together: every form of every direction and data path"""
    reached = set()
    plans = {}
    for name, c in R.CASES.items():
        for direction in R.DIRECTIONS:
            if c["forms"][direction] is None:
                continue
            p = plans[(name, direction)] = R.plan_of(name, direction)
            assert p["form"] == c["forms"][direction], (name, direction, p)
            for k, v in c["reach"].get(direction, {}).items():
                assert p[k] == v, "%s %s: %s is %r, the case list says %r" % (name, direction, k, p[k], v)
            reached.add((c["path"], direction, p["form"], c["tier"]))
    for tier in ("exact", "round"):
        have = {(pa, d, f) for pa, d, f, t in reached if t == tier}
        want = {("f32", "fwd", f) for f in ("STEM", "CONV64", "CLS", "ENGINE")} | {("f32", "dgrad", f) for f in ("CONV64", "CLS", "PARITY", "ENGINE")} \
            | {("f32", "wgrad", f) for f in ("STEM", "CONV64", "TAP", "ENGINE")} | {("b16", "fwd", f) for f in ("CONV64", "CLS", "ENGINE")} \
            | {("b16", "dgrad", f) for f in ("CONV64", "CLS", "PARITY", "ENGINE")} | {("b16", "wgrad", f) for f in ("TAP", "ENGINE")} \
            | {("opt", d, "ENGINE") for d in R.DIRECTIONS}
        assert want <= have, (tier, sorted(want - have))
    assert {("f32", d, "REFUSED", "exact") for d in R.DIRECTIONS} | {("b16", d, "REFUSED", "exact") for d in R.DIRECTIONS} <= reached
    eng = [p for p in plans.values() if p["form"] == "ENGINE"]
    assert {p["tile"] for p in eng} == {(64, 64), (128, 64), (128, 128), (256, 64)}
    assert {p["buf"] for p in eng} == {True, False} and {p["fixup"] for p in eng} == {None, "fixup", "fixup1"}
    assert any(p["streamk"] and p["split_tiles"] > 0 for p in eng) and any(not p["streamk"] and p["ntiles"] > p["G"] for p in eng)
    cls = [p for p in plans.values() if p["form"] == "CLS"]
    assert {(2, 2), (2, 3), (3, 2), (3, 3), (5, 4)} <= {p["grid"] for p in cls}
    assert {p["last_cut"] for (n, d), p in plans.items() if p["form"] == "CLS" and d == "fwd" and R.CASES[n]["d"]["stride"] == 2} \
        == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(p["s2"] for p in cls) and any(p["ragged_cols"] for p in cls) and any(p["ragged_rows"] for p in cls)
    assert {R.CASES[n]["d"]["N"] for (n, d), p in plans.items() if p["form"] in ("CLS", "TAP")} >= {128, 129, 257}
    par = [p for p in plans.values() if p["form"] == "PARITY"]
    assert any(p["dead"] == 3 for p in par) and any(sorted(t for _, _, t in p["classes"]) == [1, 2, 2, 4] for p in par)
    assert any(all(t == 4 for _, _, t in p["classes"]) for p in par) and any(all(t == 1 for _, _, t in p["classes"]) and p["dead"] == 0 for p in par)
    c64 = [p for p in plans.values() if p["form"] == "CONV64"]
    assert any(p.get("tiles_per_wg", 0) > 4 for p in c64) and any(p.get("grid") == 2 and "rows_per_wg" in p for p in c64)
    # every threshold is met from both sides by a pair of cases that differ in nothing else
    for a, b, d in (("c64-w18", "c64-w19", "wgrad"), ("stem-640x12", "stem-641x12", "fwd"), ("stem-8x68", "stem-8x72", "wgrad"),
                    ("cls-cap4", "cls-cap3", "fwd"), ("cls-cap9", "cls-cap4", "wgrad"), ("cls-3x3", "cls-n127", "fwd"),
                    ("cls-2x2", "cls-ho1", "dgrad"), ("tall", "tall-no_tall", "fwd")):
        pa, pb = plans[(a, d)], plans[(b, d)]
        assert (pa["form"], pa.get("tile")) != (pb["form"], pb.get("tile")), (a, b, d)


def test_every_exact_case_satisfies_the_2_24_condition():
    n = 0
    for name, c in R.CASES.items():
        g = R.geom(c["d"])
        assert c["K"] == dict(fwd=g.KS ** 2 * g.C, dgrad=g.KS ** 2 * g.Co, wgrad=g.N * g.Ho * g.Wo)
        assert all(64 * k + 8 < 2 ** 24 for k in c["K"].values()), name
        n += c["tier"] == "exact"
    assert n == len(R.CASES) - len(R.ROUNDING) and sorted(sum((getattr(R, grp) for grp in R.GROUPS), [])) == sorted(R.CASES)
    assert re.search(r"all (\d+) exact cases", R.__doc__).group(1) == str(n)


def test_geometry_refusals():
    """conv_geom, restated: non-positive dimensions, a negative pad, stride 3, a kernel that fits nowhere (C's division rounds
    (H + 2 pad - KS) / 2 = -1 / 2 to 0, which used to pass as Ho = 1)"""
    ok = dict(N=2, H=5, W=5, C=32, Co=32, KS=3, stride=1, pad=1)
    assert R.geom(ok) is not None
    for k in ("N", "H", "W", "C", "Co", "KS", "stride"):
        assert R.geom(dict(ok, **{k: 0})) is None and R.geom(dict(ok, **{k: -1})) is None
    assert R.geom(dict(ok, pad=-1)) is None and R.geom(dict(ok, stride=3)) is None
    assert R.geom(dict(ok, H=2, KS=3, pad=0, stride=2)) is None and R.geom(dict(ok, W=1, KS=4, pad=1, stride=2)) is None
    assert R.geom(dict(ok, H=1, KS=3, pad=1)).Ho == 1
    for direction in R.DIRECTIONS:
        assert R.conv_plan(direction, dict(ok, stride=3))["form"] == "REFUSED"


# ------------------------------------------------------------------------------------------ the float32 twin passes
def _impl(mutant=None):
    return lambda bufs, direction: R.twin(bufs, direction, mutant=mutant)


@pytest.mark.parametrize("name", R.ROUNDING)
def test_rounding_bound_is_within_reach_of_float32(name):
    ratio = R.check_conv(_impl(), name, tag=TAG)
    print("%s: worst error / bound %.4f" % (name, ratio))
    assert 0 < ratio <= 1


@pytest.mark.parametrize("group", [g for g in R.GROUPS if g != "ROUNDING"])
def test_exact_tier_holds_for_the_float32_twin(group):
    for name in getattr(R, group):
        assert R.check_conv(_impl(), name, tag=None) == 0.0


def test_bf16_rounded_operands_miss_the_rounding_bound():
    """what the bound is for: operands narrowed to bf16 on the way miss the fp32 bound by more than 2 x"""
    for name in ("round-sk", "round-k5-p4", "round-cls"):
        bufs = R.prepare(name)
        for b in ("x_buf", "dy_buf", "wf_buf", "wd_buf"):
            setattr(bufs, b, R._to_bf16(getattr(bufs, b)))
        for direction in R.DIRECTIONS:
            R.twin(bufs, direction)
            worst = float(R.scaled_error(name, direction, bufs).max())
            print("%s %s with bf16-rounded operands: %.1f x the bound" % (name, direction, worst))
            assert worst > 2.0


# ------------------------------------------------------------------------------------------ the mutants are rejected
MUTANT_CASES = [
    ("tap_dropped", "k3-s1-p1"), ("tap_dropped", "k2-s2-p1"), ("tap_dropped", "c64-5x7"), ("tap_dropped", "cls-2x3"), ("tap_dropped", "round-sk"),
    ("kernel_not_flipped", "k3-s1-p1"), ("kernel_not_flipped", "k4-s1-p2"), ("kernel_not_flipped", "par-k3-7x6"), ("kernel_not_flipped", "round-cls"),
    ("parity_neighbour", "par-k3-7x7"), ("parity_neighbour", "par-k1"), ("parity_neighbour", "par-k2"), ("parity_neighbour", "cls-s2-5x6"),
    ("parity_neighbour", "round-par-k4"),
    ("padding_live", "k3-s1-p1"), ("padding_live", "k5-s1-p2"), ("padding_live", "cls-2x2"), ("padding_live", "stem-9x12"), ("padding_live", "round-c64"),
    ("ragged_row_dropped", "tall"), ("ragged_row_dropped", "co36"), ("ragged_row_dropped", "c64-5x7"), ("ragged_row_dropped", "round-k5-p4"),
    ("dx_ignored", "sk-acc"), ("dx_ignored", "par-k1-acc"), ("dx_ignored", "c64-c2-acc"), ("dx_ignored", "round-cls"),
    ("dx_twice", "sk-acc"), ("dx_twice", "par-k4-p1-acc"), ("dx_twice", "cls-2x3"), ("dx_twice", "round-sk"),
    ("class_row_shifted", "cls-2x2"), ("class_row_shifted", "cls-3x2"), ("class_row_shifted", "b16-cls"), ("class_row_shifted", "round-cls-s2"),
    ("dw_ckk_order", "k3-s1-p1"), ("dw_ckk_order", "cls-3x3"), ("dw_ckk_order", "c64-w18"), ("dw_ckk_order", "round-sk"),
]
# the directions a mutant acts on (the others run unmutated)
ACTS_ON = dict(kernel_not_flipped=("dgrad",), parity_neighbour=("dgrad",), dx_ignored=("dgrad",), dx_twice=("dgrad",), dw_ckk_order=("wgrad",),
               ragged_row_dropped=("fwd",))


def test_every_mutant_is_listed():
    assert {m for m, _ in MUTANT_CASES} == set(R.MUTANTS)


@pytest.mark.parametrize("mutant,name", MUTANT_CASES)
def test_mutant_is_rejected(mutant, name):
    R.check_conv(_impl(), name, tag=None)                          # the same evaluation passes without the mutation
    dirs = [d for d in ACTS_ON.get(mutant, R.DIRECTIONS) if R.CASES[name]["forms"][d] not in (None, "REFUSED")]
    if mutant == "class_row_shifted":
        dirs = [d for d in dirs if R.CASES[name]["forms"][d] in ("CLS", "TAP")]
    assert dirs
    for direction in dirs:                                         # ... and fails in EVERY direction the mutation acts on
        with pytest.raises(AssertionError):
            R.check_conv(lambda bufs, d: R.twin(bufs, d, mutant=mutant if d == direction else None), name, tag=None)
