"""CPU tests of the dense-GEMM oracle (tests/gemm_ref.py): the restated plan against the source text and against what every
case claims to reach, the invariants of the share arithmetic the kernels rely on, every case of tests/test_gemm_gpu.py with
a float32 CPU evaluation in the place of the HIP path (the rounding bound is within reach of correct float32 arithmetic, in
two summation orders), and mutants of that evaluation which ``check_gemm`` must reject."""
import os
import re

import numpy as np
import pytest

import gemm_ref as R

TAG = "cpu32"


def _src(name):
    with open(os.path.join(R.CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------ the restatement against the source
def test_constants_match_the_source():
    """the constants gemm_plan aims the cases with, read back from the source text: a change there fails here"""
    igemm, streamk, gemm, common = _src("igemm.h"), _src("streamk.h"), _src("gemm.hip"), _src("common.h")
    assert int(re.search(r"constexpr int BK = (\d+);", igemm).group(1)) == R.BK
    assert int(re.search(r"constexpr int FIXUP1_DEPTH = (\d+);", streamk).group(1)) == R.FIXUP1_DEPTH
    m = re.search(r"constexpr size_t SLAB_FLOATS = \(size_t\)(\d+) \* (\d+) \* (\d+);", streamk)
    assert int(m.group(1)) * int(m.group(2)) * int(m.group(3)) == R.SLAB_FLOATS
    m = re.search(r"if \(d->M <= (\d+) \|\| d->N <= (\d+)\) return run2<64, 64>", gemm)
    assert int(m.group(1)) == int(m.group(2)) == R.SMALL_TILE_AT
    assert "return run2<128, 128>(a, b, e, d, s, slab);" in gemm
    assert "(long)d->M * d->lda < (1L << 29) - 64" in gemm and R.ROWVEC4_LIMIT == (1 << 29) - 64
    # plan_rounds' two thresholds, the resident workgroups per CU and the depth rule of launch_fixup
    assert "if (no_sk || rem * 10 >= G * 9)" in streamk
    assert "cap = iters / 4 > 0 ? iters / 4 : 1" in streamk
    assert "if ((G + rt - 1) / rt <= deep)" in streamk
    assert "else if (variant == 0) per_cu = BIG ? 2 : (BM * BN >= 128 * 64 ? 3 : 4);" in igemm
    assert "else if (variant == 1 || !BIG) per_cu = BIG ? 3 : (BM * BN >= 128 * 64 ? 4 : 6);" in igemm
    assert "const int variant = TALL ? 3 : (var >= 0 ? var : (BIG ? 2 : 1));" in igemm
    assert "return (m > 0 && m < 256) ? m : 256;" in common
    assert "for (int g = ga + 1 + wave; g <= gb; g += 16)" in streamk and "for (int g = ga + 1; g <= gb; g += 4)" in streamk
    # the operand-form conditions gemm_plan restates, one term each
    for term in ("d->lda % 4 == 0 && d->K % 4 == 0 && (uintptr_t)A % 16 == 0 && (long)d->M * d->lda < (1L << 29) - 64",
                 "(d->lda % 4 == 0) && (d->M % 4 == 0) && ((uintptr_t)A % 16 == 0)",
                 "(d->ldb % 4 == 0) && (d->N % 4 == 0) && ((uintptr_t)B % 16 == 0)",
                 "igemm::RowVec4 a{A, d->lda, d->M, d->K, d->relu_a};", "igemm::RowPlain a{A, d->lda, d->M, d->K, d->relu_a};",
                 "igemm::ColPlain<4> a{A, d->lda, d->M, d->K, d->relu_a};", "igemm::ColPlain<1> a{A, d->lda, d->M, d->K, d->relu_a};",
                 "igemm::RowPlain b{B, d->ldb, d->N, d->K, d->relu_b};", "igemm::ColPlain<4> b{B, d->ldb, d->N, d->K, d->relu_b};",
                 "igemm::ColPlain<1> b{B, d->ldb, d->N, d->K, d->relu_b};"):
        assert term in gemm, term


def test_cited_lines_hold():
    """every line number in gemm_plan's comments still holds the text it is cited for"""
    lines = {f: _src(f).split("\n") for f in {c[0] for c in R.CITES}}
    for f, n, text in R.CITES:
        assert text in lines[f][n - 1], "%s:%d no longer holds %r: move the citation in gemm_plan and in CITES" % (f, n, text)
    cited = set()
    for m in re.finditer(r"lines? (\d+)(?:-(\d+))?\)", _src_plan()):
        cited.update(int(g) for g in m.groups() if g)
    assert cited <= {n for _, n, _ in R.CITES}, sorted(cited - {n for _, n, _ in R.CITES})


def _src_plan():
    import inspect
    return inspect.getsource(R.gemm_plan)


def test_cases_reach_what_they_claim():
    """every case against gemm_plan, and what the cases must reach together"""
    plans = {}
    for name, c in R.CASES.items():
        p = plans[name] = R.plan_of(name)
        for k, v in c["reach"].items():
            assert p[k] == v, "%s: %s is %r, the case list says %r" % (name, k, p[k], v)
        if c["tier"] == "round":
            assert c["K"] <= 513
    assert {p["a_form"] for p in plans.values()} == {"RowVec4", "RowPlain", "ColPlain4", "ColPlain1"}
    assert {p["b_form"] for p in plans.values()} == {"RowPlain", "ColPlain4", "ColPlain1"}
    assert {p["tile"] for p in plans.values()} == {64, 128}
    for kern in ("fixup", "fixup1"):
        for sparse in (True, False):
            assert any(p["fixup"] == kern and p["sparse"] == sparse and p["split_tiles"] > 0 for p in plans.values()), (kern, sparse)
        assert any(p["fixup"] == kern and p["second_iter"] and not p["sparse"] for p in plans.values()), kern
    assert any(p["empty_inside"] for p in plans.values())
    assert any(p["interior"] and p["edge"] for p in plans.values())
    assert any(p["G"] % 8 != 0 and p["G"] > 8 for p in plans.values())
    assert any(p["partial_round"] for p in plans.values())
    assert any(p["rem"] > 0 and p["split_tiles"] == 0 for p in plans.values())
    assert any(p["kchunks"] > 1 for p in plans.values())
    assert any(p["full_rounds"] == 0 and p["rem"] > 0 for p in plans.values()) and any(p["full_rounds"] >= 4 for p in plans.values())
    # the scalar forms are reached all three ways, for each transposition
    for t in ("tA0-tB0", "tA0-tB1", "tA1-tB0", "tA1-tB1"):
        forms = {k: (plans["form-%s-%s" % (t, k)]["a_form"], plans["form-%s-%s" % (t, k)]["b_form"])
                 for k in ("vec", "pad4", "pad5", "off", "dims")}
        assert forms["vec"] == forms["pad4"] and forms["pad5"] == forms["off"] == forms["dims"] and forms["vec"][0] != forms["pad5"][0]
        # each way is the ONLY cause in its case: (dimension, ld, base) of A and, where B is not transposed, of B
        for k, only in (("pad5", "ld"), ("off", "base"), ("dims", "dim")):
            c = R.CASES["form-%s-%s" % (t, k)]
            d = R.descriptor(c)
            conds = [dict(dim=(d["M"] if c["tA"] else d["K"]) % 4 == 0, ld=d["lda"] % 4 == 0, base=c["offa"] == 0)]
            if not c["tB"]:
                conds.append(dict(dim=d["N"] % 4 == 0, ld=d["ldb"] % 4 == 0, base=c["offb"] == 0))
            for cond in conds:
                assert [w for w, ok in cond.items() if not ok] == [only], (t, k, cond)
            if k == "dims":                                  # NaN padding right behind the last k / m / n of every row
                assert d["lda"] > (d["M"] if c["tA"] else d["K"]) and d["ldb"] > (d["K"] if c["tB"] else d["N"])
    # the slab indices the kernels use stay inside the workspace
    assert all(p["G"] * p["tile"] ** 2 <= R.SLAB_FLOATS for p in plans.values())


def test_every_option_value_changes_a_plan():
    """each swept option value changes the restated plan of at least one case it is applied to"""
    changed = {}
    for name, option, value, base in R.OPTION_SWEEP:
        assert R.CASES[name]["opts"][option] == value
        a, b = R.plan_of(name), R.plan_of(base)
        changed[(option, value)] = changed.get((option, value), False) or a != b
    assert set(changed) == {("no_streamk", 1), ("no_streamk", 10), ("no_streamk", 11), ("no_streamk", 12), ("no_fixup1", 1),
                            ("no_fixup1", 3), ("igemm_variant", 0), ("igemm_variant", 1), ("igemm_variant", 2), ("stagger", 1),
                            ("bf16", 1), ("bf16", 2), ("kmajor", 1), ("max_cus", 5)}
    same = sorted(k for k, v in changed.items() if not v)
    # igemm_variant = 2 is the 128-tile's default and means variant 1 on 64-tiles: it can change no dense plan
    assert same == [("igemm_variant", 2)], same
    # max_cus aims most of the table: every value used there gives that case a plan of its own (but 200x64x40, whose 8
    # iterations cap G at 2 on any number of CUs)
    for name in R.TABLE:
        if "max_cus" in R.CASES[name]["opts"] and name != "200x64x40-c1":
            assert R.plan_of(name) != R.plan_of(name, max_cus=None), name


# ------------------------------------------------------------------------------------------ the share arithmetic
def test_share_owner_inverts_lo_hi():
    """gemm_ref's share_lo / share_hi / share_owner (what gemm_plan and the twin use): owner(it) is the g with
    lo(g) <= it < hi(g); the shares tile [0, R) in order (what the kernels' walk and the fix-up kernels' cut must agree
    on), exhaustively for R <= 300, G <= 80"""
    for G in range(1, 81):
        g = np.arange(G)
        for Rr in range(1, 301):
            lo, hi = R.share_lo(g, Rr, G), R.share_hi(g, Rr, G)
            assert lo[0] == 0 and hi[-1] == Rr and (lo[1:] == hi[:-1]).all() and (hi >= lo).all()
            it = np.arange(Rr)
            own = R.share_owner(it, Rr, G)
            assert (0 <= own).all() and (own < G).all() and (lo[own] <= it).all() and (it < hi[own]).all(), (Rr, G)
    assert R.share_owner(5, 7, 3) == 2 and R.share_lo(2, 7, 3) == 4 and R.share_hi(2, 7, 3) == 7


def test_xcd_remap_is_a_bijection():
    """gemm_ref.xcd_remap (common.h's, restated) for every grid size a dense product can have"""
    for G in range(1, 1537):
        assert np.array_equal(np.sort(R.xcd_remap(np.arange(G), G)), np.arange(G)), G
    assert [int(R.xcd_remap(b, 14)) for b in range(14)] == [0, 2, 4, 6, 8, 10, 12, 13, 1, 3, 5, 7, 9, 11]
    assert "return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;" in _src("common.h")


# ------------------------------------------------------------------------------------------ the float32 twin passes
def _impl(order, mutant=None):
    return lambda bufs, d: R.twin(bufs, d, order=order, mutant=mutant)


@pytest.mark.parametrize("order", ["numpy", "shares"])
@pytest.mark.parametrize("name", R.ROUNDING)
def test_rounding_bound_is_within_reach_of_float32(name, order):
    ratio = R.check_gemm(_impl(order), name, tag=TAG + "-" + order)
    print("%s %s: worst error / bound %.4f" % (name, order, ratio))
    assert 0 < ratio <= 1


@pytest.mark.parametrize("group", ["TABLE", "FORMS", "EPILOGUES", "RELU", "OPTION_SWEEP"])
def test_exact_tier_holds_for_the_float32_twin(group):
    names = getattr(R, group)
    names = [n[0] for n in names] + R.OPTION_BASES if group == "OPTION_SWEEP" else names
    for name in names:
        for order in (("numpy", "shares") if group in ("TABLE", "EPILOGUES") else ("shares",)):
            assert R.check_gemm(_impl(order), name, tag=None) == 0.0


def test_bf16_rounded_operands_miss_the_rounding_bound():
    """what the bound is for: operands narrowed to bf16 on the way miss it by more than 2 x at K <= 513"""
    for name in ("round-300x333x513-c3", "round-37x130x33", "round-384x384x96-c4"):
        bufs = R.prepare(name)
        bufs.A_buf, bufs.B_buf = R._to_bf16(bufs.A_buf), R._to_bf16(bufs.B_buf)
        R.twin(bufs, bufs.d)
        worst = float(R.scaled_error(name, bufs).max())
        print("%s with bf16-rounded operands: %.1f x the bound" % (name, worst))
        assert worst > 2.0


# ------------------------------------------------------------------------------------------ the mutants are rejected
MUTANT_CASES = [
    ("drop_ktile", "300x333x513-c3"), ("drop_ktile", "300x333x513-c1-nows"), ("drop_ktile", "round-300x333x513-c3"),
    ("slab_twice", "384x384x640-c4"), ("slab_twice", "640x256x64-c4"), ("slab_twice", "round-384x384x96-c4"),
    ("empty_slab", "384x384x96-c4"), ("empty_slab", "98371x64x40"),
    ("bias_every_piece", "epi-bias-split-tile"), ("bias_every_piece", "epi-bias-deep"), ("bias_every_piece", "round-300x333x513-c3"),
    ("c_twice", "epi-acc"), ("c_twice", "epi-acc-split4"), ("c_twice", "round-64x64x512"),
    ("relu_skipped", "relu-tA0-tB0-pad4-a1b0"), ("relu_skipped", "relu-tA1-tB1-pad5-a0b1-bf16"), ("relu_skipped", "round-37x130x33"),
    ("relu_other", "relu-tA0-tB0-pad4-a1b0"), ("relu_other", "relu-tA1-tB0-pad5-a0b1"), ("relu_other", "round-64x64x512"),
    ("row_stride", "form-tA0-tB0-vec"), ("row_stride", "form-tA1-tB0-pad5"), ("row_stride", "round-384x384x96-c4"),
    ("c_padding_written", "form-tA0-tB0-pad4"), ("c_padding_written", "form-tA0-tB0-vec"), ("c_padding_written", "round-300x333x513-c3"),
    ("nan_padding", "form-tA0-tB0-pad5"), ("nan_padding", "form-tA1-tB1-pad4"), ("nan_padding", "form-tA0-tB1-vec"),
    ("nan_padding", "form-tA0-tB0-dims"),           # what a 16-byte fetch at the last k of a row would do with lda % 4 == 0, K % 4 != 0
    ("k_mult4", "300x333x513-c3"), ("k_mult4", "37x130x1"), ("k_mult4", "round-300x333x513-c3"),
]


def test_every_mutant_is_listed():
    assert {m for m, _ in MUTANT_CASES} == set(R.MUTANTS)


@pytest.mark.parametrize("mutant,name", MUTANT_CASES)
def test_mutant_is_rejected(mutant, name):
    R.check_gemm(_impl("shares"), name, tag=None)                 # the same evaluation passes without the mutation
    with pytest.raises(AssertionError):
        R.check_gemm(_impl("shares", mutant), name, tag=None)
