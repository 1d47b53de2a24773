"""The oracle of the dense-GEMM tests (``avvad_gemm_f32``: csrc/gemm.hip -> ``igemm::launch`` in csrc/igemm.h, schedule and
fix-ups in csrc/streamk.h): the float64 reference, the buffers with their sentinel padding, the launch plan RESTATED
(``gemm_plan``), the case list, a float32 CPU twin with its mutants, and ONE assertion function, ``check_gemm``.  It takes
the implementation under test as a callable ``impl(bufs, d)`` that receives the prepared buffers and the descriptor and
returns nothing (the result is what it leaves in ``bufs.C_buf``): tests/test_gemm_gpu.py passes the HIP path through ctypes,
tests/test_gemm_cpu.py passes the float32 twin (the bound must be within reach of correct float32 arithmetic) and mutants
of it (every assertion must be able to fail).

Reference.  C_ref = [C0 if accumulate] + relu?(op A) relu?(op B) + [bias], in float64, from the LOGICAL operands.

Two tiers of operands.

* EXACT (every schedule, option and edge case).  Entries of A, B, bias and C0 are integers in -8 .. 8 (magnitude uniform in
  0 .. 8, one third of them negative so that the ReLU matters).  With K <= 4096 every partial sum stays below
  64 x 4096 + 16 = 2^18 + 16 < 2^24: every fp32 product, every MFMA chain, every slab and every fix-up sum is exact in ANY order,
  the integers are exact in bf16 too, and so the assertion is equality with the float64 reference cast to float32 -- for
  fp32, for options bf16 = 1 and 2, and for the K-major cells' float atomics.  No tolerance: a dropped or doubled K tile, a
  slab nobody wrote, a bias added twice on a split tile or an old C added twice cannot hide.
* ROUNDING (a handful of cases, K <= 513).  Operands N(0, 1); |got - ref|[m, n] <= (K + 40) 2^-24 S[m, n] with
  S = |op A| |op B| + |bias| + |C0| in float64 (absolute values AFTER the ReLU where one is asked for): gamma_K of one ordered
  chain of K products (unit round-off 2^-24) plus at most 32 more additions (the pieces of a split tile, the bias, the old
  C) and head-room of 8 for the second-order terms.  Derived, not measured, and with no aggregate alternative.  Operands
  rounded to bf16 on the way (8 bits of mantissa: a relative 2^-9 per product) miss it by more than 2 x at K <= 513; under
  options bf16 = 1 and 2 the operands are therefore PRE-ROUNDED to bf16 (value-pinned) and the same bound holds.

Guards.  Every buffer carries sentinel padding.  A and B: the columns beyond the logical extent inside lda / ldb and a
guard block before and after hold NaN -- padding that enters a product poisons it.  C: the columns N .. ldc-1 and the guard
blocks hold the bit pattern of -0.0f and must be bit-identical afterwards.  (-0.0 is the one value that even ``+= 0.0f``
changes: the fix-up kernels add a slab sum, which is +0 for a column beyond N, and a NaN or a finite non-zero sentinel
would survive that.)

Measured.  The exact tier has no figure: all 198 exact cases are equal to the float64 product on the MI355X, bit-identical run
to run, and so are the two cases around RowVec4's 2 GiB switch over all 2^20 rows.  Rounding tier, worst error / bound,
MI355X | float32 CPU twin in numpy's order | in share order:
  round-300x333x513-c3          0.0079 | 0.0047 | 0.0047        round-37x130x33             0.0459 | 0.0459 | 0.0459
  round-300x333x513-c4-tt-acc   0.0089 | 0.0050 | 0.0050        round-300x332x512-nows      0.0089 | 0.0053 | 0.0053
  round-384x384x96-c4           0.0378 | 0.0378 | 0.0378        round-300x333x513-c3-bf16   0.0027 | 0.0018 | 0.0018
  round-64x64x512               0.0019 | 0.0031 | 0.0019        round-64x64x512-bf16-2      0.0009 | 0.0021 | 0.0009
(the bound is the worst case of K aligned rounding errors; random ones add up to its square root.  The figures that agree
to four digits are elements with one dominant product, where only the final rounding is left.)  The same twin on operands
rounded to bf16 misses the bound by 25 x (K = 513), 213 x (K = 96) and 720 x (K = 33)
(tests/test_gemm_cpu.py::test_bf16_rounded_operands_miss_the_rounding_bound).
"""
import functools
import os
import types
import zlib

import numpy as np

import head_ref as H

FAMILY = "gemm"
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "audio-visual-vad_amd", "csrc")

# constants of the engine; tests/test_gemm_cpu.py::test_constants_match_the_source reads them back from the source text
BK = 32                                   # igemm.h: constexpr int BK
FIXUP1_DEPTH = 6                          # streamk.h: constexpr int FIXUP1_DEPTH
SLAB_FLOATS = 256 * 576 * 64              # streamk.h: constexpr size_t SLAB_FLOATS
SMALL_TILE_AT = 64                        # gemm.hip run1: M <= 64 || N <= 64 -> 64x64 tiles
ROWVEC4_LIMIT = (1 << 29) - 64            # gemm.hip: (long)M * lda < (1L << 29) - 64 keeps RowVec4's byte offsets below 2^31
EINVAL = -1

GUARD = 256                               # floats of guard in front of and behind every buffer (1 KiB: keeps 16-byte alignment)
SENTINEL = np.uint32(0x80000000)          # -0.0f
OPTIONS = ("max_cus", "no_streamk", "no_fixup1", "igemm_variant", "stagger", "bf16", "kmajor")
DESC_FIELDS = ("M", "N", "K", "lda", "ldb", "ldc", "transA", "transB", "accumulate", "split_k", "relu_a", "relu_b")


# ------------------------------------------------------------------------------------------ the plan, restated
# The lines gemm_plan's comments cite, as (file, line, text that line must hold): tests/test_gemm_cpu.py::test_cited_lines_hold
# fails when an edit of the engine moves one, so the citations cannot drift unnoticed.
CITES = [
    ("gemm.hip", 16, "if (d->M <= 64 || d->N <= 64) return run2<64, 64>"),
    ("gemm.hip", 22, "if (d->transB) {"),
    ("gemm.hip", 26, "const bool v4 = (d->ldb % 4 == 0) && (d->N % 4 == 0) && ((uintptr_t)B % 16 == 0);"),
    ("gemm.hip", 32, "return run1(a, b, e, d, s, slab);"),
    ("gemm.hip", 40, "d->split_k > 1 ? 2 : (d->accumulate ? 1 : 0)"),
    ("gemm.hip", 42, "if (!d->transA) {"),
    ("gemm.hip", 43, "if (d->lda % 4 == 0 && d->K % 4 == 0 && (uintptr_t)A % 16 == 0 && (long)d->M * d->lda < (1L << 29) - 64) {"),
    ("gemm.hip", 50, "const bool v4 = (d->lda % 4 == 0) && (d->M % 4 == 0) && ((uintptr_t)A % 16 == 0);"),
    ("gemm.hip", 56, "return runA(a, B, e, d, s, slab);"),
    ("gemm.hip", 63, "ws_bytes >= igemm::SLAB_FLOATS * sizeof(float)"),
    ("igemm.h", 890, "const int ktiles = (K + BK - 1) / BK;"),
    ("igemm.h", 896, "const int variant = TALL ? 3 : (var >= 0 ? var : (BIG ? 2 : 1));"),
    ("igemm.h", 902, "else per_cu = 2;"),
    ("igemm.h", 909, "if (split_k_hint > 1 && e.mode != 0 && ntiles <= plan.G && tn.kmajor) {"),
    ("igemm.h", 920, "if ((long)kchunks * ntiles < plan.G) plan.G = (long)kchunks * ntiles;"),
    ("igemm.h", 954, "if (rt > 0) launch_fixup<BM, BN>("),
    ("streamk.h", 322, "static inline long workers(int per_cu, int BM, int BN) {"),
    ("streamk.h", 325, "return G;"),
    ("streamk.h", 334, "static inline Rounds plan_rounds(long ntiles, int ktiles, long G, bool slab, int mode) {"),
    ("streamk.h", 338, "if (no_sk || rem * 10 >= G * 9) {"),
    ("streamk.h", 343, "cap = iters / 4 > 0 ? iters / 4 : 1"),
    ("streamk.h", 346, "return Rounds{G, (int)full_rounds, (int)rem};"),
    ("streamk.h", 373, "if ((G + rt - 1) / rt <= deep)"),
    ("streamk.h", 376, "hipLaunchKernelGGL((fixup<BM, BN, Epi>)"),
]


def share_lo(g, R, G):                    # streamk.h Share::lo
    return g * R // G


def share_hi(g, R, G):                    # streamk.h Share::hi
    return (g + 1) * R // G


def share_owner(it, R, G):                # streamk.h Share::owner
    return ((it + 1) * G + R - 1) // R - 1


def xcd_remap(bid, nblk):                 # common.h xcd_remap  (bid: an int or an integer array)
    q, r, x, j = nblk >> 3, nblk & 7, bid & 7, bid >> 3
    return np.where(x < r, x * (q + 1), r * (q + 1) + (x - r) * q) + j


def _cdiv(a, b):
    return -(-a // b)


def gemm_plan(d, a_aligned=True, b_aligned=True, ws=True, tile=None, **opt):
    """What ``avvad_gemm_f32`` launches for descriptor ``d`` (a dict of DESC_FIELDS), restated from the source; ``a_aligned`` /
    ``b_aligned``: the base pointer is 16-byte aligned; ``ws``: a workspace of avvad_engine_workspace() bytes is given; ``opt``:
    the options of OPTIONS that are not at their defaults.  ``tile``: the plan of a caller that instantiates
    ``igemm::launch<tile, tile>`` itself, whatever M and N are (the STFT, tests/stft_ref.py); None: the entry point's own rule."""
    assert set(opt) <= set(OPTIONS), opt
    M, N, K = d["M"], d["N"], d["K"]
    p = {}
    # gemm.hip avvad_gemm_impl (lines 42-56): the A operand
    if not d["transA"]:
        v4 = d["lda"] % 4 == 0 and K % 4 == 0 and a_aligned and M * d["lda"] < ROWVEC4_LIMIT
        p["a_form"] = "RowVec4" if v4 else "RowPlain"
    else:
        p["a_form"] = "ColPlain4" if d["lda"] % 4 == 0 and M % 4 == 0 and a_aligned else "ColPlain1"
    # gemm.hip runA (lines 22-32): the B operand
    if d["transB"]:
        p["b_form"] = "RowPlain"
    else:
        p["b_form"] = "ColPlain4" if d["ldb"] % 4 == 0 and N % 4 == 0 and b_aligned else "ColPlain1"
    # gemm.hip run1 (line 16): the tile
    BM = BN = tile if tile is not None else (64 if (M <= SMALL_TILE_AT or N <= SMALL_TILE_AT) else 128)
    big = BM == 128
    p["tile"] = BM
    # gemm.hip avvad_gemm_impl (line 40): the epilogue mode
    mode = 2 if d["split_k"] > 1 else (1 if d["accumulate"] else 0)
    p["mode"] = mode
    # igemm.h launch (lines 890-902): variant, kernel instantiation, resident workgroups per CU
    ktiles = _cdiv(K, BK)
    ntm, ntn = _cdiv(M, BM), _cdiv(N, BN)
    ntiles = ntm * ntn
    var = opt.get("igemm_variant", -1)
    variant = var if var >= 0 else (2 if big else 1)
    if variant == 0:
        per_cu, kern = (2 if big else 4), "db256"
    elif variant == 1 or not big:
        per_cu, kern = (3 if big else 6), "sb256"
    else:
        per_cu, kern = 2, "db512"
    p["kernel"], p["per_cu"] = kern, per_cu
    # streamk.h workers (lines 322-325) with common.h grid_cus
    cus = opt.get("max_cus", 0)
    cus = cus if 0 < cus < 256 else 256
    G = cus * per_cu
    if G * BM * BN > SLAB_FLOATS:
        G = SLAB_FLOATS // (BM * BN)
    slab = bool(ws)                        # gemm.hip avvad_gemm_f32 (line 63)
    kchunks = 0
    if d["split_k"] > 1 and mode != 0 and ntiles <= G and opt.get("kmajor", 0):      # igemm.h launch (lines 909-920)
        best = -1
        for r in (1, 2):
            nc = max(min(r * G // ntiles, ktiles), 1)
            rr = _cdiv(nc * ntiles, G)
            cost = rr * _cdiv(ktiles, nc) + rr * 8
            if best < 0 or cost < best:
                best, kchunks = cost, nc
        G = min(G, kchunks * ntiles)
        fr = rem = 0
    else:                                  # streamk.h plan_rounds (lines 334-346)
        nsk = opt.get("no_streamk", 0)
        no_sk = (not slab) or nsk == 1 or nsk == 10 + mode or not (float(ntiles) * ktiles * G < 4.0e9)
        fr = ntiles // G
        rem = ntiles - fr * G
        if no_sk or rem * 10 >= G * 9:
            fr, rem = fr + (1 if rem > 0 else 0), 0
        if rem > 0 and fr == 0:
            G = min(G, max(ntiles * ktiles // 4, 1))
    R = rem * ktiles
    p.update(ktiles=ktiles, ntm=ntm, ntn=ntn, ntiles=ntiles, G=G, full_rounds=fr, rem=rem, R=R, kchunks=kchunks,
             partial_round=bool(rem == 0 and kchunks == 0 and ntiles % G != 0),
             sparse=bool(rem > 0 and R < G), g_mod8=G % 8)
    # streamk.h Share::cut per pool tile; launch_fixup (lines 373-376) with igemm.h launch (line 954)
    cuts = []
    for tr in range(rem):
        cuts.append((share_owner(tr * ktiles, R, G), share_owner(tr * ktiles + ktiles - 1, R, G)))
    wrote = lambda g: share_hi(g, R, G) > share_lo(g, R, G)     # noqa: E731   (Share::wrote)
    p["cuts"] = cuts
    p["split_tiles"] = sum(1 for ga, gb in cuts if gb > ga)
    p["slabs"] = max([sum(1 for g in range(ga + 1, gb + 1) if wrote(g)) for ga, gb in cuts] or [0])
    p["empty_inside"] = any(not wrote(g) for ga, gb in cuts for g in range(ga + 1, gb))
    p["fixup"] = None
    p["second_iter"] = False
    if rem > 0:
        nf = opt.get("no_fixup1", 0)
        deep = 0 if nf == 1 else (nf if nf > 1 else FIXUP1_DEPTH)
        p["fixup"] = "fixup1" if (G + rem - 1) // rem <= deep else "fixup"
        # fixup: wave 0 walks ga+1, +16, ...; fixup1: ga+1, +4, ...: the loop body runs a second time from that many workers on
        step = 4 if p["fixup"] == "fixup1" else 16
        p["second_iter"] = any(gb - ga > step for ga, gb in cuts)
    # igemm.h kernel, the `fast` store path: interior tiles (whole tile inside M x N, M * ldc < 2^31) store without range checks
    fast_ok = M * d["ldc"] < (1 << 31)
    p["interior"] = bool(fast_ok and M >= BM and N >= BN)
    p["edge"] = bool(M % BM != 0 or N % BN != 0 or not fast_ok)
    p["bf"] = bool(opt.get("bf16", 0))                                   # igemm.h launch: bf = allow_bf16 && tn.bf16
    p["stagger"] = bool(opt.get("stagger", 0)) and kern == "db512"       # igemm.h kernel: NTH == 512 && stagger
    return p


# ------------------------------------------------------------------------------------------ the cases
CASES = {}


def _case(name, M, N, K, why, reach=None, **kw):
    c = dict(M=M, N=N, K=K, tA=0, tB=0, pa=0, pb=0, pc=0, offa=0, offb=0, acc=0, split_k=1, bias=0, relu_a=0, relu_b=0, ws=1,
             opts={}, tier="exact", why=why, reach=reach or {})
    assert set(kw) <= set(c), kw
    c.update(kw)
    assert name not in CASES, name
    assert c["tier"] == "round" and K <= 513 or c["tier"] == "exact" and K <= 4096
    CASES[name] = c
    return name


def _c(n):
    return {"max_cus": n}


# ---- the schedule table.  ``reach``: the fields of gemm_plan the case is there for (test_cases_reach_what_they_claim).
TABLE = [
    _case("64x64x2048", 64, 64, 2048, "64-tile, no full round, G capped to iters / 4 = 16, 15 slabs on the four-wave fix-up",
          dict(tile=64, full_rounds=0, G=16, slabs=15, fixup="fixup", second_iter=False)),
    _case("65x65x2048", 65, 65, 2048, "one step over the tile rule: 128-tile, one ragged tile cut 16 ways",
          dict(tile=128, full_rounds=0, rem=1, G=16, slabs=15, fixup="fixup", interior=False, edge=True)),
    _case("64x64x4096", 64, 64, 4096, "31 slabs: the second g += 16 iteration of fixup",
          dict(tile=64, G=32, slabs=31, fixup="fixup", second_iter=True)),
    _case("133x135x4096", 133, 135, 4096, "4 ragged 128-tiles, each cut 32 ways; interior and edge tiles in one launch",
          dict(tile=128, rem=4, G=128, slabs=31, second_iter=True, interior=True, edge=True)),
    _case("48x1x1024", 48, 1, 1024, "N = 1", dict(tile=64, b_form="ColPlain1", a_form="RowVec4")),
    _case("1x48x1024", 1, 48, 1024, "M = 1", dict(tile=64, b_form="ColPlain4")),
    _case("37x130x1", 37, 130, 1, "K = 1", dict(ktiles=1, a_form="RowPlain", b_form="ColPlain1")),
    _case("37x130x31", 37, 130, 31, "a K tail below one K tile", dict(ktiles=1)),
    _case("37x130x33", 37, 130, 33, "a K tail above one K tile", dict(ktiles=2)),
    _case("384x384x64-c4", 384, 384, 64, "one full round, then a sparse pool: R = 2 iterations on G = 8 workers, four-wave fix-up",
          dict(tile=128, G=8, full_rounds=1, rem=1, R=2, sparse=True, fixup="fixup", split_tiles=1), opts=_c(4)),
    _case("384x384x96-c4", 384, 384, 96, "sparse, with empty shares BETWEEN the tile's first and last worker",
          dict(G=8, R=3, sparse=True, empty_inside=True, fixup="fixup", slabs=2), opts=_c(4)),
    _case("384x384x640-c4", 384, 384, 640, "dense pool of one tile, 7 slabs", dict(G=8, R=20, sparse=False, slabs=7, fixup="fixup"),
          opts=_c(4)),
    _case("640x256x64-c4", 640, 256, 64, "sparse pool on the one-wave fix-up: rem = 2, R = 4 < G = 8",
          dict(G=8, rem=2, R=4, sparse=True, fixup="fixup1", split_tiles=2), opts=_c(4)),
    _case("300x333x513-c4", 300, 333, 513, "ragged M, N and K; one pool tile cut 8 ways", dict(G=8, rem=1, slabs=7, fixup="fixup"),
          opts=_c(4)),
    _case("300x333x513-c3", 300, 333, 513, "fixup1 with 3 split tiles", dict(G=6, rem=3, fixup="fixup1", split_tiles=3, slabs=1),
          opts=_c(3)),
    _case("300x333x513-c1", 300, 333, 513, "4 full data-parallel rounds and a one-tile pool on G = 2",
          dict(G=2, full_rounds=4, rem=1, fixup="fixup1"), opts=_c(1)),
    _case("500x60x100-c1", 500, 60, 100, "64-tile, one full round, fixup1", dict(tile=64, G=6, full_rounds=1, rem=2, fixup="fixup1"),
          opts=_c(1)),
    _case("448x64x1100-c1", 448, 64, 1100, "5 slabs: the second g += 4 iteration of fixup1",
          dict(tile=64, G=6, rem=1, slabs=5, fixup="fixup1", second_iter=True), opts=_c(1)),
    _case("130x130x1056-c7", 130, 130, 1056, "G = 14, not a multiple of 8: xcd_remap with a remainder; 4 split tiles",
          dict(G=14, g_mod8=6, rem=4, split_tiles=4), opts=_c(7)),
    _case("200x64x40-c1", 200, 64, 40, "a pool in which no tile is split: the fix-up has nothing to add",
          dict(tile=64, rem=4, split_tiles=0, fixup="fixup1"), opts=_c(1)),
    _case("98371x64x40", 98371, 64, 40, "sparse at the default G = 1536 (64-tile)",
          dict(tile=64, G=1536, full_rounds=1, rem=2, sparse=True)),
    _case("66000x128x40", 66000, 128, 40, "sparse at the default G = 512 (128-tile)",
          dict(tile=128, G=512, full_rounds=1, rem=4, sparse=True)),
    _case("300x333x513-c1-nows", 300, 333, 513, "ws = NULL: whole tiles, 9 tiles on 2 workers, a partially filled last round",
          dict(G=2, full_rounds=5, rem=0, partial_round=True, fixup=None), opts=_c(1), ws=0),
]

# ---- the descriptor sweep.  SV: every dimension and every tight ld a multiple of 4 (the vector forms are available), ragged
# against the 128-tile and the K tile; SS: no dimension a multiple of 4 (the scalar forms by shape).  Both on 3 CUs: 9 tiles
# on G = 6, one full round and three pool tiles cut in two (fixup1).  S64: the same on 64-tiles, 4 tiles on 6 workers.
SV, SS, S64 = (300, 332, 516), (301, 333, 513), (60, 200, 260)
FORMS = []
for _tA in (0, 1):
    for _tB in (0, 1):
        _t = "tA%d-tB%d" % (_tA, _tB)
        _a4 = "ColPlain4" if _tA else "RowVec4"
        _a1 = "ColPlain1" if _tA else "RowPlain"
        _b4, _b1 = ("RowPlain", "RowPlain") if _tB else ("ColPlain4", "ColPlain1")
        FORMS += [
            _case("form-%s-vec" % _t, *SV, "vector forms, tight strides", dict(a_form=_a4, b_form=_b4, fixup="fixup1", split_tiles=3),
                  tA=_tA, tB=_tB, opts=_c(3)),
            _case("form-%s-pad4" % _t, *SV, "vector forms, every ld padded by 4", dict(a_form=_a4, b_form=_b4),
                  tA=_tA, tB=_tB, pa=4, pb=4, pc=4, opts=_c(3)),
            _case("form-%s-pad5" % _t, *SV, "scalar forms by ld % 4: every ld padded by 5", dict(a_form=_a1, b_form=_b1),
                  tA=_tA, tB=_tB, pa=5, pb=5, pc=5, opts=_c(3)),
            _case("form-%s-off" % _t, *SV, "scalar forms by a base 4 bytes off its 16-byte alignment", dict(a_form=_a1, b_form=_b1),
                  tA=_tA, tB=_tB, offa=1, offb=1, opts=_c(3)),
            # (padded by 3: lda = 516 or 304, ldb = 336 or 516 -- every ld a multiple of 4 and the bases aligned, so the SHAPE
            #  alone decides; with lda % 4 == 0 a 16-byte fetch at the last k of a row would pull NaN padding into the product)
            _case("form-%s-dims" % _t, *SS, "scalar forms by K % 4, M % 4 and N % 4 ALONE: ld % 4 == 0, aligned bases",
                  dict(a_form=_a1, b_form=_b1), tA=_tA, tB=_tB, pa=3, pb=3, pc=3, opts=_c(3)),
            _case("form64-%s-vec" % _t, *S64, "64-tile, vector forms, ld padded by 4", dict(tile=64, a_form=_a4, b_form=_b4, fixup="fixup1"),
                  tA=_tA, tB=_tB, pa=4, pb=4, pc=4, opts=_c(1)),
            _case("form64-%s-pad5" % _t, *S64, "64-tile, scalar forms by ld % 4", dict(tile=64, a_form=_a1, b_form=_b1),
                  tA=_tA, tB=_tB, pa=5, pb=5, pc=5, opts=_c(1)),
        ]

# ---- epilogues, on SS / c=3 (three split pool tiles and six whole ones) unless stated; C padded by 5
EPILOGUES = [
    _case("epi-acc", *SS, "accumulate onto a given C", dict(mode=1, split_tiles=3), acc=1, pc=5, opts=_c(3)),
    _case("epi-acc-split4", *SS, "accumulate + split_k = 4 (mode 2)", dict(mode=2, split_tiles=3), acc=1, split_k=4, pc=5, opts=_c(3)),
    _case("epi-bias-split-tile", *SS, "bias where tiles are split: only the piece that starts a tile's K range may add it",
          dict(mode=0, split_tiles=3), bias=1, pc=5, opts=_c(3)),
    _case("epi-bias-acc", *SS, "bias and accumulate together", dict(mode=1), bias=1, acc=1, pc=5, opts=_c(3)),
    _case("epi-bias-whole", 200, 64, 40, "bias with no split tile (a pool of whole tiles)", dict(split_tiles=0, rem=4), bias=1, pc=5,
          opts=_c(1)),
    _case("epi-bias-nows", *SS, "bias on the whole-tile schedule", dict(rem=0), bias=1, pc=5, opts=_c(3), ws=0),
    _case("epi-bias-deep", 64, 64, 2048, "bias on a tile cut 16 ways (four-wave fix-up)", dict(slabs=15, fixup="fixup"), bias=1, pc=4),
    _case("epi-acc-sparse", 384, 384, 96, "accumulate on a sparse pool with empty shares inside the tile", dict(empty_inside=True), acc=1,
          opts=_c(4)),
]

# ---- the fused ReLU: relu_a, relu_b and both, on every operand form (vector and scalar-by-ld of each transposition), fp32 and
# bf16 = 1.  One third of the exact tier's entries are negative, so a skipped or misplaced ReLU changes every element.
RELU = []
for _tA in (0, 1):
    for _tB in (0, 1):
        for _pad in (4, 5):
            for _ra, _rb in ((1, 0), (0, 1), (1, 1)):
                for _bf in (0, 1):
                    _o = dict(max_cus=3, **({"bf16": 1} if _bf else {}))
                    RELU.append(_case("relu-tA%d-tB%d-pad%d-a%db%d%s" % (_tA, _tB, _pad, _ra, _rb, "-bf16" if _bf else ""), *SV,
                                      "ReLU fused into the operand staging", dict(bf=bool(_bf)), tA=_tA, tB=_tB, pa=_pad, pb=_pad,
                                      pc=_pad, relu_a=_ra, relu_b=_rb, opts=_o))

# ---- the option sweep, on split-tile cases of the table (no_streamk = 10 + mode and kmajor need their epilogue mode)
_SPLIT = ["64x64x2048", "133x135x4096", "384x384x96-c4", "640x256x64-c4", "300x333x513-c3", "448x64x1100-c1"]
OPTION_SWEEP = []          # (case name, option, value, name of the same case without that option)
OPTION_BASES = []          # the comparison cases that are not in the table: its rows with accumulate / split_k = 4


def _opt_case(base, option, value, **kw):
    b = CASES[base]
    name = "%s%s-%s%d" % (base, "".join("-%s%d" % (k, v) for k, v in sorted(kw.items())), option, value)
    opts = dict(b["opts"], **{option: value})
    fields = {k: b[k] for k in ("tA", "tB", "pa", "pb", "pc", "acc", "split_k", "bias", "ws")}
    fields.update(kw)
    _case(name, b["M"], b["N"], b["K"], "%s under option %s = %d" % (base, option, value), {}, opts=opts, **fields)
    if kw:                                 # the comparison case: same descriptor, option at its default
        tb = "%s%s" % (base, "".join("-%s%d" % (k, v) for k, v in sorted(kw.items())))
        if tb not in CASES:
            OPTION_BASES.append(_case(tb, b["M"], b["N"], b["K"], base + " with " + str(kw), {}, opts=dict(b["opts"]), **fields))
    else:
        tb = base
    OPTION_SWEEP.append((name, option, value, tb))
    return name


for _b in _SPLIT:
    _opt_case(_b, "no_streamk", 1)
    _opt_case(_b, "no_streamk", 10)
    _opt_case(_b, "no_streamk", 11, acc=1)
    _opt_case(_b, "no_streamk", 12, acc=1, split_k=4)
    for _v in (1, 3):
        _opt_case(_b, "no_fixup1", _v)
    for _v in (0, 1, 2):
        _opt_case(_b, "igemm_variant", _v)
    _opt_case(_b, "stagger", 1)
    for _v in (1, 2):
        _opt_case(_b, "bf16", _v)
    _opt_case(_b, "kmajor", 1, acc=1, split_k=4)
_opt_case("300x333x513-c3", "max_cus", 5)       # (max_cus is what aims every other row; here it is the swept option)

# ---- the rounding tier
ROUNDING = [
    _case("round-300x333x513-c3", 300, 333, 513, "ragged, three split tiles, bias", bias=1, pc=5, opts=_c(3), tier="round"),
    _case("round-300x333x513-c4-tt-acc", 300, 333, 513, "TT, accumulate, 8-way split tile", tA=1, tB=1, acc=1, pa=5, opts=_c(4),
          tier="round"),
    _case("round-384x384x96-c4", 384, 384, 96, "sparse pool, vector forms", opts=_c(4), tier="round"),
    _case("round-64x64x512", 64, 64, 512, "64-tile cut 4 ways, relu_a, bias, accumulate", relu_a=1, bias=1, acc=1, tier="round"),
    _case("round-37x130x33", 37, 130, 33, "short K, relu_b, transposed B", tB=1, relu_b=1, tier="round"),
    _case("round-300x332x512-nows", 300, 332, 512, "whole tiles: one ordered chain of 512 per element", tA=1, ws=0, tier="round"),
    _case("round-300x333x513-c3-bf16", 300, 333, 513, "bf16 = 1 on operands pre-rounded to bf16", bias=1, opts=dict(max_cus=3, bf16=1),
          tier="round"),
    _case("round-64x64x512-bf16-2", 64, 64, 512, "bf16 = 2 on operands pre-rounded to bf16, relu_a", relu_a=1, acc=1,
          opts=dict(bf16=2), tier="round"),
]


# ------------------------------------------------------------------------------------------ buffers and reference
def descriptor(c):
    M, N, K = c["M"], c["N"], c["K"]
    return dict(M=M, N=N, K=K, lda=(M if c["tA"] else K) + c["pa"], ldb=(K if c["tB"] else N) + c["pb"], ldc=N + c["pc"],
                transA=c["tA"], transB=c["tB"], accumulate=c["acc"], split_k=c["split_k"], relu_a=c["relu_a"], relu_b=c["relu_b"])


def plan_of(name, **override):
    c = CASES[name]
    opts = dict(c["opts"], **override)
    return gemm_plan(descriptor(c), a_aligned=c["offa"] == 0, b_aligned=c["offb"] == 0, ws=bool(c["ws"]),
                     **{k: v for k, v in opts.items() if v is not None})


def _to_bf16(x):
    import torch
    return torch.from_numpy(x).bfloat16().float().numpy()


def _draw(rng, tier, *shape):
    if tier == "exact":
        mag = rng.integers(0, 9, shape).astype(np.float32)
        return np.where(rng.random(shape) < 1.0 / 3.0, -mag, mag).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


@functools.lru_cache(maxsize=8)
def _inputs(name):
    """the logical operands of a case (float32): A as stored (rows x cols), B as stored, bias or None, C0"""
    c = CASES[name]
    M, N, K = c["M"], c["N"], c["K"]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    A = _draw(rng, c["tier"], *((K, M) if c["tA"] else (M, K)))
    B = _draw(rng, c["tier"], *((N, K) if c["tB"] else (K, N)))
    if c["tier"] == "round" and c["opts"].get("bf16"):
        A, B = _to_bf16(A), _to_bf16(B)                   # value-pinned: what the bf16 staging would round to
    bias = _draw(rng, c["tier"], N) if c["bias"] else None
    C0 = _draw(rng, c["tier"], M, N)
    return A, B, bias, C0


@functools.lru_cache(maxsize=8)
def reference(name):
    """(C_ref, S) in float64"""
    c = CASES[name]
    A, B, bias, C0 = _inputs(name)
    a = (A.T if c["tA"] else A).astype(np.float64)
    b = (B.T if c["tB"] else B).astype(np.float64)
    if c["relu_a"]:
        a = np.maximum(a, 0)
    if c["relu_b"]:
        b = np.maximum(b, 0)
    ref = a @ b
    S = np.abs(a) @ np.abs(b)
    if c["acc"]:
        ref, S = ref + C0, S + np.abs(C0)
    if bias is not None:
        ref, S = ref + bias, S + np.abs(bias)
    return ref, S


def _padded(X, ld, off, fill):
    """flat float32 buffer [GUARD + off][rows x ld][GUARD]: X in the leading columns of each row, ``fill`` everywhere else"""
    rows, cols = X.shape
    buf = np.full(GUARD + off + rows * ld + GUARD, fill, dtype=np.float32)
    buf[GUARD + off:GUARD + off + rows * ld].reshape(rows, ld)[:, :cols] = X
    return buf


def prepare(name):
    """fresh buffers of a case: A_buf / B_buf (NaN padding and guards), C_buf (-0.0 padding and guards, C0 in the logical
    positions whether or not the case accumulates), bias, the float offsets a0 / b0 / c0 of the base pointers, the descriptor"""
    c = CASES[name]
    A, B, bias, C0 = _inputs(name)
    d = descriptor(c)
    minus0 = np.float32(-0.0)
    return types.SimpleNamespace(name=name, d=d, case=c, A_buf=_padded(A, d["lda"], c["offa"], np.nan),
                                 B_buf=_padded(B, d["ldb"], c["offb"], np.nan), C_buf=_padded(C0, d["ldc"], 0, minus0),
                                 bias=None if bias is None else bias.copy(), a0=GUARD + c["offa"], b0=GUARD + c["offb"], c0=GUARD,
                                 ws=bool(c["ws"]))


def c_view(bufs):
    d = bufs.d
    return bufs.C_buf[bufs.c0:bufs.c0 + d["M"] * d["ldc"]].reshape(d["M"], d["ldc"])


def check_gemm(impl, name, tag="gpu"):
    """``impl(bufs, d)`` runs the product on ``bufs`` (see ``prepare``) and leaves the result in ``bufs.C_buf``.  Checked: every
    float of C outside the logical M x N keeps the sentinel's bits; exact tier: the result EQUALS the float64 reference cast to
    float32; rounding tier: |got - ref| <= (K + 40) 2^-24 S element-wise.  Returns the worst error / bound (0 for the exact tier)."""
    c = CASES[name]
    bufs = prepare(name)
    ref, S = reference(name)
    M, N, K = c["M"], c["N"], c["K"]
    impl(bufs, bufs.d)
    bits = bufs.C_buf.view(np.uint32).copy()
    keep = np.ones(bits.shape, dtype=bool)
    keep[bufs.c0:bufs.c0 + M * bufs.d["ldc"]].reshape(M, bufs.d["ldc"])[:, :N] = False
    bad = np.flatnonzero(keep & (bits != SENTINEL))
    assert bad.size == 0, "%s: %d floats of C outside the %d x %d output were written, the first at float %d of the buffer " \
        "(row %d, column %d of the [M][ldc] block)" % (name, bad.size, M, N, bad[0], (bad[0] - bufs.c0) // bufs.d["ldc"],
                                                       (bad[0] - bufs.c0) % bufs.d["ldc"])
    got = c_view(bufs)[:, :N].astype(np.float64)
    assert np.isfinite(got).all(), "%s: %d non-finite elements (operand padding multiplied in?), the first at %s" % (
        name, int((~np.isfinite(got)).sum()), tuple(np.argwhere(~np.isfinite(got))[0]))
    if c["tier"] == "exact":
        assert float(np.abs(ref).max()) < 2 ** 24 and np.array_equal(ref, np.round(ref))
        wrong = np.argwhere(got != ref)
        assert wrong.size == 0, "%s: %d of %d elements differ from the exact product; the first at (m, n) = %s: got %r, exact %r; " \
            "rows %d .. %d, columns %d .. %d" % (name, len(wrong), M * N, tuple(wrong[0]), got[tuple(wrong[0])], ref[tuple(wrong[0])],
                                                  wrong[:, 0].min(), wrong[:, 0].max(), wrong[:, 1].min(), wrong[:, 1].max())
        return 0.0
    scaled = scaled_error(name, bufs)
    return H.report(FAMILY, name + " |d| / ((K + 40) 2^-24 S)", scaled, np.zeros_like(scaled), 1.0, tag=tag)


def scaled_error(name, bufs):
    """|got - ref| / ((K + 40) 2^-24 S) per element (0 / 0 = 0; an error where the bound is 0 counts as 1e30)"""
    ref, S = reference(name)
    got = c_view(bufs)[:, :CASES[name]["N"]].astype(np.float64)
    bound = (CASES[name]["K"] + 40) * 2.0 ** -24 * S
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / bound, np.where(err == 0, 0.0, 1e30))


# ------------------------------------------------------------------------------------------ the float32 CPU twin
MUTANTS = ("drop_ktile", "slab_twice", "empty_slab", "bias_every_piece", "c_twice", "relu_skipped", "relu_other", "row_stride",
           "c_padding_written", "nan_padding", "k_mult4")


def _gather(buf, base, rows, cols, stride):
    idx = base + np.arange(rows)[:, None] * stride + np.arange(cols)[None, :]
    return buf[np.clip(idx, 0, buf.size - 1)]


def twin(bufs, d, order="numpy", mutant=None):
    """float32 evaluation on the prepared buffers.  ``order`` "numpy": one float32 product; "shares": the tiles of the stream-K
    pool are evaluated piece by piece as ``gemm_plan`` cuts them -- the piece that starts a tile's K range lands on the output
    (with the old C and the bias), the others are summed in the fix-up kernel's order (fixup1: ascending workers; fixup: wave w
    takes every fourth worker, the four wave sums meet in wave order) and added onto it.  ``mutant``: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    c = bufs.case
    M, N, K = d["M"], d["N"], d["K"]
    f32 = np.float32
    extra = 1 if mutant == "nan_padding" else 0
    sa = d["lda"] + (1 if mutant == "row_stride" else 0)
    if d["transA"]:
        a = _gather(bufs.A_buf, bufs.a0, K + extra, M, sa).T
    else:
        a = _gather(bufs.A_buf, bufs.a0, M, K + extra, sa)
    if d["transB"]:
        b = _gather(bufs.B_buf, bufs.b0, N, K + extra, d["ldb"]).T
    else:
        b = _gather(bufs.B_buf, bufs.b0, K + extra, N, d["ldb"])
    Kc = K + extra
    if mutant == "k_mult4":
        Kc = K // 4 * 4
    ra, rb = d["relu_a"], d["relu_b"]
    if mutant == "relu_skipped":
        ra = rb = 0
    if mutant == "relu_other":
        ra, rb = rb, ra
    a = np.ascontiguousarray(np.maximum(a, 0) if ra else a, dtype=f32)[:, :Kc]
    b = np.ascontiguousarray(np.maximum(b, 0) if rb else b, dtype=f32)[:Kc]
    Cv = c_view(bufs)
    old = Cv[:, :N].copy()
    mode = d["accumulate"] or d["split_k"] > 1
    bias = bufs.bias if bufs.bias is not None else None

    def land(prod, m0, m1, n0, n1):                     # the kernel's store: old + acc + bias, or acc + bias
        v = prod
        if mode:
            v = old[m0:m1, n0:n1] + v
            if mutant == "c_twice":
                v = v + old[m0:m1, n0:n1]
        if bias is not None:
            v = v + bias[n0:n1]
        return v.astype(f32)

    out = land(a @ b, 0, M, 0, N)
    p = gemm_plan(d, a_aligned=c["offa"] == 0, b_aligned=c["offb"] == 0, ws=bufs.ws, **c["opts"])
    needs_pool = mutant in ("slab_twice", "empty_slab", "bias_every_piece")
    if order == "shares" or mutant == "drop_ktile" or needs_pool:
        BMN, kt, G, R = p["tile"], p["ktiles"], p["G"], p["R"]
        assert not needs_pool or p["split_tiles"] > 0, "mutant %s needs a split tile" % mutant
        done = False
        tiles = [(p["full_rounds"] * G + tr, cut) for tr, cut in enumerate(p["cuts"])]
        if mutant == "drop_ktile" and not tiles:
            tiles = [(0, (0, 0))]
        for t, (ga, gb) in tiles:
            m0, n0 = (t // p["ntn"]) * BMN, (t % p["ntn"]) * BMN
            m1, n1 = min(m0 + BMN, M), min(n0 + BMN, N)
            tr = t - p["full_rounds"] * G
            pieces = []                                  # (worker, first K tile, one past the last) inside this tile
            if p["rem"] > 0:
                for g in range(ga, gb + 1):
                    lo, hi = max(share_lo(g, R, G), tr * kt), min(share_hi(g, R, G), (tr + 1) * kt)
                    pieces.append((g, lo - tr * kt, hi - tr * kt))
            else:
                pieces.append((0, 0, kt))
            assert sum(k1 - k0 for _, k0, k1 in pieces if k1 > k0) == kt and pieces[0][2] > pieces[0][1]

            def prod(k0, k1):
                return a[m0:m1, k0 * BK:min(k1 * BK, Kc)] @ b[k0 * BK:min(k1 * BK, Kc), n0:n1]
            g0, k0, k1 = pieces[0]
            if mutant == "drop_ktile" and not done:
                k0, done = k0 + 1, True
            tile = land(prod(k0, k1), m0, m1, n0, n1)
            slabs = []                                   # (place in the fix-up's walk = worker - (ga + 1), partial sums)
            for g, k0, k1 in pieces[1:]:
                pos = g - (ga + 1)
                if k1 <= k0:                             # an empty share: nothing written, nothing to add
                    if mutant == "empty_slab" and not done:
                        slabs.append((pos, np.full((m1 - m0, n1 - n0), 3.0, dtype=f32)))
                        done = True
                    continue
                s = prod(k0, k1)
                if mutant == "bias_every_piece" and bias is not None:
                    s = s + bias[n0:n1]
                slabs.append((pos, s.astype(f32)))
                if mutant == "slab_twice" and not done:
                    slabs.append((pos, s.astype(f32)))
                    done = True
            if slabs:
                if p["fixup"] == "fixup1":
                    tot = np.zeros_like(tile)
                    for _, s in slabs:
                        tot = tot + s
                else:                                    # wave w sums the workers ga + 1 + w, + 4, ...; the sums meet in wave order
                    waves = [np.zeros_like(tile) for _ in range(4)]
                    for pos, s in slabs:
                        waves[pos % 4] = waves[pos % 4] + s
                    tot = ((waves[0] + waves[1]) + waves[2]) + waves[3]
                tile = tile + tot
            out[m0:m1, n0:n1] = tile
        assert mutant not in ("drop_ktile", "slab_twice", "empty_slab") or done, "mutant %s found no place to act" % mutant
        assert mutant != "bias_every_piece" or bias is not None
    Cv[:, :N] = out
    if mutant == "c_padding_written":
        if d["ldc"] > N:
            Cv[M // 2, N] = 0.0
        else:
            bufs.C_buf[bufs.c0 + M * d["ldc"]] = 0.0


def log_worst(tag):
    H.log_worst(tag)
