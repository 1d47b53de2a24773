"""The oracle of the single-convolution tests (``avvad_conv2d_{pack_weights,fwd,dgrad,wgrad}`` and their ``_bf16`` twins:
csrc/trunk.hip -> igemm.h / conv_ops.h / conv64.h / bgemm.h): the float64 reference in the ABI's layouts, the buffers with
their guard blocks, the kernel-form choice RESTATED (``conv_plan``), the case list, a float32 CPU twin (a plain im2col in
numpy, per direction) with its mutants, and ONE assertion function, ``check_conv``.  It takes the implementation under test
as a callable ``impl(bufs, direction) -> rc`` that runs one direction ("fwd", "dgrad", "wgrad") on the prepared buffers and
leaves the result in ``bufs.y_buf`` / ``bufs.dx_buf`` / ``bufs.dw_buf``: tests/test_conv_gpu.py passes the HIP path through
ctypes, tests/test_conv_cpu.py passes the float32 twin and mutants of it (every assertion must be able to fail).

Reference.  F.conv2d and autograd in float64 on the CPU from the LOGICAL operands (x NCHW, w OIHW, dy NCHW), expressed in the
ABI's layouts: NHWC activations, dw_packed[(kh, kw, c)][co], dgrad with ``accumulate`` = dx0 + dgrad.

Two tiers of operands.

* EXACT (every schedule, option and edge case).  Entries of x, w, dy and the old dx are integers in -8 .. 8.  The case
  builder asserts 64 K + 8 < 2^24 for the contraction length K of every direction (forward KS^2 C, dgrad KS^2 Co, wgrad
  N Ho Wo): every fp32 product, MFMA chain, slab, per-workgroup partial and fix-up sum is then exact in ANY order, the values
  are exact in bf16 too, and the assertion is equality with the float64 reference cast to float32 -- for the fp32 entry
  points, for them under option bf16 = 1, and for the _bf16 entry points.  No tolerance: a dropped tap or K tile, a slab added
  twice, a class row that reads its neighbour's pixel or image, a parity class with the wrong taps cannot hide.
* ROUNDING (a handful of cases per direction and data path).  Operands N(0, 1), on the bf16 paths pre-rounded to bf16;
  |got - ref| <= (K + A + 8) 2^-24 S element-wise, S the same convolution of |x| and |w| (|dy| and |w|; |x| and |dy|; + |dx0|
  when accumulating) in float64, K the contraction length, A the extra additions the restated plan gives an element: the
  pieces of a split tile (the slabs of the stream-K pool, bounded for the position-class and tap schedules by
  ceil(longest tile / smallest share) + 1), the per-workgroup partials of the conv64 and stem weight gradients, the old dx
  (and the zero-filled dx under the four parity-class launches).  Derived, not measured; no aggregate alternative.

Guards.  Every operand and output buffer carries a guard block before and after it.  Input guards hold NaN: a guard element
that enters a product poisons it.  Output guards hold the bit pattern of -0.0f and must be bit-identical after the call; the
logical part of y and dw starts as NaN (an element nobody writes shows), dx starts as dx0 whether or not the case
accumulates.  The GPU test refills the engine scratch with NaN before every launch, runs every case twice (bit-identical) and
checks that the inputs are unchanged.  A refusal (form "REFUSED") must return AVVAD_EINVAL and leave every bit of the output
buffer as it was.

Measured.  The exact tier has no figure: all 120 exact cases are equal to the float64
reference on the MI355X and bit-identical run to run.  Rounding tier, worst error / bound over the case's directions,
MI355X | float32 CPU twin:
  round-sk             0.0080 | 0.0051      round-sk-no_fixup1   0.0095 | 0.0049      round-k5-p4          0.0083 | 0.0135
  round-par-k4         0.0736 | 0.0736      round-stem           0.0535 | 0.0535      round-c64            0.0083 | 0.0048
  round-cls            0.0014 | 0.0022      round-cls-s2         0.0049 | 0.0049      round-sk-bf16opt     0.0034 | 0.0020
  round-b16-sk         0.0026 | 0.0019      round-b16-cls        0.0008 | 0.0013      round-b16-c64        0.0025 | 0.0027
  round-b16-par        0.0272 | 0.0394
(the bound is the worst case of K aligned rounding errors; random ones add up to its square root.  The figures that agree to
four digits are elements with a few dominant products -- the weight gradient of a 4x4 / 2 kernel over 48 pixels, the stem's 49
taps -- where only the final rounding is left.)  The same twin on operands rounded to bf16 misses the fp32 bound by 3.6 .. 82 x
(tests/test_conv_cpu.py::test_bf16_rounded_operands_miss_the_rounding_bound).
"""
import functools
import os
import types
import zlib

import numpy as np

import gemm_ref as G
import head_ref as H

FAMILY = "conv"
CSRC = G.CSRC
EINVAL = -1
GUARD = 256                               # floats (or bf16 pairs' worth: 1 KiB) of guard in front of and behind every buffer
SENTINEL = np.uint32(0x80000000)          # -0.0f
DESC_FIELDS = ("N", "H", "W", "C", "Co", "KS", "stride", "pad")
OPTIONS = ("max_cus", "no_streamk", "no_fixup1", "no_buf", "no_tall", "no_cls", "no_s2_cls", "cls_cap", "no_conv64",
           "no_stem_kernel", "bf16")
DIRECTIONS = ("fwd", "dgrad", "wgrad")
FORMS = ("STEM", "CONV64", "CLS", "TAP", "PARITY", "ENGINE")

# constants of the launchers; tests/test_conv_cpu.py::test_constants_match_the_source reads them back from the source text
WG_MAXW = 18                              # conv64.h: widest grid row of the conv64 weight-gradient kernel
WG_PART = 576 * 64                        # conv64.h: floats per partial of that kernel
STEM_WH = 17                              # trunk.hip: Wo / 2 the stem weight-gradient kernel's register rows hold
STEM_LDS = 48 * 1024                      # trunk.hip stem_kernel_ok: the padded frame's LDS budget
CLS_TILES_PER_CU = 4                      # trunk.hip cls_tile_cap
FITS_BUF = (1 << 29) - 64                 # trunk.hip fits_buf
FITS_U30 = 1 << 30                        # trunk.hip fits_u30

# The lines conv_plan's comments cite, as (file, line, text that line must hold): tests/test_conv_cpu.py::test_cited_lines_hold
CITES = [
    ("trunk.hip", 539, 'static inline bool fits_u30(long n) { return n >= 0 && n < (1L << 30); }'),
    ("trunk.hip", 541, 'static inline bool taps_fit(const Geom& g) { return g.KS * g.KS <= 32; }'),
    ("trunk.hip", 543, 'static inline bool fits_buf(long n_floats) { return n_floats >= 0 && n_floats < (1L << 29) - 64; }'),
    ("trunk.hip", 545, 'static inline bool stem_kernel_ok(const Geom& g) {'),
    ("trunk.hip", 547, 'return g.C == 1 && g.KS == 7 && g.stride == 2 && g.pad == 3 && g.Co == 64 && (size_t)(g.H + 6) * LDW * sizeof(float) <= 48 * 1024 &&'),
    ("trunk.hip", 552, 'return stem_kernel_ok(g) && (g.Wo & 1) == 0 && g.Wo <= 2 * STEM_WH && slab && (long)g.Ho * g.Wo * 64 * 4 < (1L << 31);'),
    ("trunk.hip", 558, 'return 4L * grid_cus();'),
    ("trunk.hip", 562, 'return avvad_tune().bf16 == 0 && !avvad_tune().no_cls && slab && g.KS == 3 && g.pad == 1 && g.N >= 128 && g.C % 32 == 0 &&'),
    ("trunk.hip", 567, 'if (!cls_common(g, slab) || g.Co % 4 || g.Co < 128) return false;'),
    ("trunk.hip", 575, 'if (!cls_common(g, slab) || (g.stride != 1 && (g.stride != 2 || avvad_tune().no_s2_cls)) || g.C % 4 || g.C < 128) return false;'),
    ("trunk.hip", 582, 'if (!cls_common(g, slab) || g.C % 128 || g.Co % 4 || g.Co < 128) return false;'),
    ("trunk.hip", 590, 'return (b16 || avvad_tune().bf16 == 0) && !avvad_tune().no_conv64 && g.C == 64 && g.Co == 64 && g.KS == 3 && g.stride == 1 &&'),
    ("trunk.hip", 596, 'return conv64_ok(g, false) && slab && g.W <= conv64::WG_MAXW && (size_t)grid_cus() * conv64::WG_PART <= igemm::SLAB_FLOATS &&'),
    ("trunk.hip", 606, 'return g.C % 64 == 0 && g.Co % 64 == 0 && taps_fit(g) && fits_buf((long)g.N * g.H * g.W * g.C / 2) &&'),
    ("trunk.hip", 614, 'return !avvad_tune().no_cls && slab && g.KS == 3 && g.pad == 1 && g.N >= 128 && g.Ho >= 2 && g.Wo >= 2 && g.Ho * g.Wo <= 9 &&'),
    ("trunk.hip", 618, 'if (!cls16_common(g, slab) || g.Co < 128) return false;'),
    ("trunk.hip", 625, ': g.stride == 2 && g.KS == 3 && g.pad == 1 && !avvad_tune().no_cls && !avvad_tune().no_s2_cls &&'),
    ("trunk.hip", 630, 'return cls16_common(g, slab) && g.C % 128 == 0 && g.Co >= 128 && 9L * (g.C / 128) * cdiv(g.Co, 128) <= cls_tile_cap();'),
    ("trunk.hip", 646, 'static ConvForm fwd_form(const Geom& g, bool b16, bool slab) {'),
    ("trunk.hip", 652, 'if (g.C == 1) return stem_kernel_ok(g) ? ConvForm{STEM, 0, 0, false, g.N} : ConvForm{ENGINE, 128, 64, false, 0};'),
    ("trunk.hip", 653, 'const int rows = g.Co <= 64 && !avvad_tune().no_tall ? 256 : 128;'),
    ("trunk.hip", 657, 'static ConvForm dgrad_form(const Geom& g, bool b16, bool slab) {'),
    ("trunk.hip", 662, 'if (g.stride == 2) return {PARITY, 128, cols, buf};'),
    ("trunk.hip", 663, 'return {ENGINE, cols == 64 && !b16 && !avvad_tune().no_tall ? 256 : 128, cols, buf};'),
    ("trunk.hip", 665, 'static ConvForm wgrad_form(const Geom& g, bool b16, bool slab) {'),
    ("trunk.hip", 667, 'if (b16) return conv_wgrad16_tap_ok(g, slab) ? ConvForm{TAP} : ConvForm{ENGINE, 128, cols, true};'),
    ("trunk.hip", 670, 'if (g.C == 1) return stem_wgrad_ok(g, slab) ? ConvForm{STEM} : ConvForm{ENGINE, 64, 64, false};'),
    ("trunk.hip", 677, 'const int lsh = ((g.Ho - 1) * g.stride - g.pad + 2 > g.H - 1) ? 1 : 0, lsw = ((g.Wo - 1) * g.stride - g.pad + 2 > g.W - 1) ? 1 : 0;'),
    ("trunk.hip", 767, 'if (g.Co % 4) return AVVAD_EINVAL;'),
    ("trunk.hip", 773, 'if (g.C % 32 || g.Co % 4 || !taps_fit(g)) return AVVAD_EINVAL;'),
    ("trunk.hip", 782, 'if (b16 && !bf16_conv_ok(g)) return AVVAD_EINVAL;'),
    ("trunk.hip", 833, 'if (ntap > 4) return AVVAD_EINVAL;'),
    ("trunk.hip", 836, 'if (!accumulate) hipLaunchKernelGGL(zero_f32, dim3(ew_grid(n)), dim3(256), 0, s, dx, n);'),
    ("trunk.hip", 854, 'if (g.Co % 32 || g.C % 4 || !taps_fit(g)) return AVVAD_EINVAL;'),
    ("trunk.hip", 880, 'if (b16 && !bf16_conv_ok(g)) return AVVAD_EINVAL;'),
    ("trunk.hip", 910, 'if (!B16 && g.Co % 4) return AVVAD_EINVAL;'),
    ("trunk.hip", 921, 'if (g.C % 32) return AVVAD_EINVAL;'),
    ("trunk.hip", 934, 'if (!bf16_conv_ok(g)) return AVVAD_EINVAL;'),
    ("trunk.hip", 941, 'const int nb = g.N < 256 ? g.N : 256;'),
    ("trunk.hip", 950, 'const int grid = NR < grid_cus() ? NR : grid_cus();'),
    ("trunk.hip", 1083, 'if (d->H + 2 * d->pad < d->KS || d->W + 2 * d->pad < d->KS) return false;'),
    ("trunk.hip", 1085, 'if (Ho <= 0 || Wo <= 0 || (d->stride != 1 && d->stride != 2)) return false;'),
    ("trunk.hip", 1172, 'if (!w_oihw || !wf16 || !conv_geom(d, &g) || g.C % 64 || g.Co % 64) return AVVAD_EINVAL;'),
    ("streamk.h", 385, 'G = workers(2, 128, 128);'),
    ("streamk.h", 388, 'if (G > R / 4) G = R / 4 > 0 ? R / 4 : 1;'),
    ("conv64.h", 346, 'static inline int grid_for(long M, int cus) {'),
    ("bgemm.h", 389, 'const igemm::Rounds plan = igemm::plan_rounds(ntiles, ktiles, igemm::workers(2, BM, BN), slab != nullptr, e.mode);'),
]


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------ the plan, restated
def geom(d):
    """trunk.hip conv_geom (lines 1083-1085): the descriptor with Ho and Wo, or None where every entry point refuses it"""
    N, Hh, W, C, Co, KS, s, p = (d[k] for k in DESC_FIELDS)
    if min(N, Hh, W, C, Co, KS, s) <= 0 or p < 0:
        return None
    if Hh + 2 * p < KS or W + 2 * p < KS or s not in (1, 2):
        return None
    g = types.SimpleNamespace(**{k: d[k] for k in DESC_FIELDS})
    g.Ho, g.Wo = (Hh + 2 * p - KS) // s + 1, (W + 2 * p - KS) // s + 1
    return g


def _grid_cus(opt):
    m = opt.get("max_cus", 0)
    return m if 0 < m < 256 else 256


def _fits_buf(n):
    return 0 <= n < FITS_BUF


def _taps_fit(g):
    return g.KS * g.KS <= 32


def _cls_tile_cap(opt):                   # trunk.hip cls_tile_cap (line 558)
    return opt["cls_cap"] if opt.get("cls_cap", 0) > 0 else CLS_TILES_PER_CU * _grid_cus(opt)


def _stem_kernel_ok(g, opt):              # (lines 545-547)
    ldw = (g.W + 6) | 1
    return (g.C == 1 and g.KS == 7 and g.stride == 2 and g.pad == 3 and g.Co == 64 and (g.H + 6) * ldw * 4 <= STEM_LDS
            and not opt.get("no_stem_kernel", 0))


def _stem_wgrad_ok(g, slab, opt):         # (line 552)
    return _stem_kernel_ok(g, opt) and g.Wo % 2 == 0 and g.Wo <= 2 * STEM_WH and slab and g.Ho * g.Wo * 64 * 4 < (1 << 31)


def _cls_common(g, slab, opt):            # (line 562)
    return (opt.get("bf16", 0) == 0 and not opt.get("no_cls", 0) and slab and g.KS == 3 and g.pad == 1 and g.N >= 128
            and g.C % 32 == 0 and g.Co % 32 == 0 and g.Ho >= 2 and g.Wo >= 2 and not opt.get("no_buf", 0)
            and opt.get("no_streamk", 0) == 0)


def _fwd_cls_ok(g, slab, opt):            # (line 567)
    if not _cls_common(g, slab, opt) or g.Co % 4 or g.Co < 128:
        return False
    return (g.Ho * g.Wo * _cdiv(g.N, 128) * _cdiv(g.Co, 128) <= _cls_tile_cap(opt) and _fits_buf(g.N * g.H * g.W * g.C)
            and _fits_buf(9 * g.C * g.Co))


def _dgrad_cls_ok(g, slab, opt):          # (line 575)
    if not _cls_common(g, slab, opt) or (g.stride != 1 and (g.stride != 2 or opt.get("no_s2_cls", 0))) or g.C % 4 or g.C < 128:
        return False
    return (g.H * g.W * _cdiv(g.N, 128) * _cdiv(g.C, 128) <= _cls_tile_cap(opt) and _fits_buf(g.N * g.Ho * g.Wo * g.Co)
            and _fits_buf(9 * g.C * g.Co))


def _wgrad_tap_ok(g, slab, opt):          # (line 582)
    if not _cls_common(g, slab, opt) or g.C % 128 or g.Co % 4 or g.Co < 128:
        return False
    return (9 * (g.C // 128) * _cdiv(g.Co, 128) <= _cls_tile_cap(opt) and _fits_buf(g.N * g.H * g.W * g.C)
            and _fits_buf(g.N * g.Ho * g.Wo * g.Co))


def _conv64_ok(g, b16, opt):              # (line 590)
    M = g.N * g.H * g.W
    return ((b16 or opt.get("bf16", 0) == 0) and not opt.get("no_conv64", 0) and g.C == 64 and g.Co == 64 and g.KS == 3
            and g.stride == 1 and g.pad == 1 and g.Ho == g.H and g.Wo == g.W and M > 0 and _fits_buf(M * 64)
            and (M + 64) * (g.H * g.W) < (1 << 32))


def _conv64_wgrad_ok(g, slab, opt):       # (line 596)
    return (_conv64_ok(g, False, opt) and slab and g.W <= WG_MAXW and _grid_cus(opt) * WG_PART <= G.SLAB_FLOATS
            and g.N * g.H * g.W * 256 < (1 << 31))


def _bf16_conv_ok(g):                     # (line 606)
    return (g.C % 64 == 0 and g.Co % 64 == 0 and _taps_fit(g) and _fits_buf(g.N * g.H * g.W * g.C // 2)
            and _fits_buf(g.N * g.Ho * g.Wo * g.Co // 2) and _fits_buf(g.KS * g.KS * g.C * g.Co // 2))


def _cls16_common(g, slab, opt):          # (line 614)
    return (not opt.get("no_cls", 0) and slab and g.KS == 3 and g.pad == 1 and g.N >= 128 and g.Ho >= 2 and g.Wo >= 2
            and g.Ho * g.Wo <= 9 and opt.get("no_streamk", 0) == 0)


def _fwd16_cls_ok(g, slab, opt):          # (line 618)
    return (_cls16_common(g, slab, opt) and g.Co >= 128
            and g.Ho * g.Wo * _cdiv(g.N, 128) * _cdiv(g.Co, 128) <= _cls_tile_cap(opt))


def _dgrad16_cls_ok(g, slab, opt):        # (line 625)
    if g.stride == 1:
        form = _cls16_common(g, slab, opt)
    else:
        form = (g.stride == 2 and g.KS == 3 and g.pad == 1 and not opt.get("no_cls", 0) and not opt.get("no_s2_cls", 0)
                and opt.get("no_streamk", 0) == 0 and slab and g.N >= 128)
    return form and g.C >= 128 and g.H * g.W * _cdiv(g.N, 128) * _cdiv(g.C, 128) <= _cls_tile_cap(opt)


def _wgrad16_tap_ok(g, slab, opt):        # (line 630)
    return (_cls16_common(g, slab, opt) and g.C % 128 == 0 and g.Co >= 128
            and 9 * (g.C // 128) * _cdiv(g.Co, 128) <= _cls_tile_cap(opt))


def _workers(per_cu, BM, BN, opt):        # streamk.h workers
    Gw = _grid_cus(opt) * per_cu
    return min(Gw, G.SLAB_FLOATS // (BM * BN)) if Gw * BM * BN > G.SLAB_FLOATS else Gw


def engine_rounds(M, N, K, BM, BN, b16, ws, mode, opt):
    """igemm::launch / bgemm::launch (bgemm.h line 389) for one product on BM x BN tiles: the stream-K rounds.  For the square
    tiles of the fp32 engine this IS gemm_ref.gemm_plan (asserted); the 128 x 64 and 256 x 64 tiles and the bf16 engine restate
    the same rules with their own resident-workgroup counts."""
    ktiles, ntm, ntn = _cdiv(K, G.BK), _cdiv(M, BM), _cdiv(N, BN)
    ntiles = ntm * ntn
    if b16 or BM == 256:
        per_cu = 2
    elif BM == 128 and BN == 128:
        per_cu = 2
    else:
        per_cu = 4 if BM * BN >= 128 * 64 else 6
    Gw = _workers(per_cu, BM, BN, opt)
    nsk = opt.get("no_streamk", 0)
    no_sk = (not ws) or nsk == 1 or nsk == 10 + mode or not (float(ntiles) * ktiles * Gw < 4.0e9)
    fr = ntiles // Gw
    rem = ntiles - fr * Gw
    if no_sk or rem * 10 >= Gw * 9:
        fr, rem = fr + (1 if rem > 0 else 0), 0
    if rem > 0 and fr == 0:
        Gw = min(Gw, max(ntiles * ktiles // 4, 1))
    R = rem * ktiles
    cuts = [(G.share_owner(tr * ktiles, R, Gw), G.share_owner(tr * ktiles + ktiles - 1, R, Gw)) for tr in range(rem)]
    wrote = lambda g: G.share_hi(g, R, Gw) > G.share_lo(g, R, Gw)     # noqa: E731
    slabs = max([sum(1 for g in range(ga + 1, gb + 1) if wrote(g)) for ga, gb in cuts] or [0])
    fixup = None
    if rem > 0:
        nf = opt.get("no_fixup1", 0)
        deep = 0 if nf == 1 else (nf if nf > 1 else G.FIXUP1_DEPTH)
        fixup = "fixup1" if (Gw + rem - 1) // rem <= deep else "fixup"
    p = dict(tile=(BM, BN), ktiles=ktiles, ntiles=ntiles, G=Gw, full_rounds=fr, rem=rem, slabs=slabs, fixup=fixup,
             split_tiles=sum(1 for ga, gb in cuts if gb > ga), ragged=bool(M % BM != 0), streamk=bool(rem > 0))
    if not b16 and BM == BN and BM in (64, 128):
        q = G.gemm_plan(dict(M=M, N=N, K=K, lda=K, ldb=N, ldc=N, transA=0, transB=0, accumulate=mode, split_k=1, relu_a=0, relu_b=0),
                        ws=ws, tile=BM, **{k: v for k, v in opt.items() if k in ("max_cus", "no_streamk", "no_fixup1")})
        assert all(q[k] == p[k] for k in ("G", "full_rounds", "rem", "slabs", "fixup", "split_tiles")), (p, q)
    return p


def _pool(R, ntiles, maxlen, opt):
    """streamk.h plan_cls (lines 385-388): every tile is in the stream-K pool; a tile of ``maxlen`` K tiles meets at most
    ceil(maxlen / smallest share) + 1 shares"""
    Gw = _workers(2, 128, 128, opt)
    if Gw > R // 4:
        Gw = max(R // 4, 1)
    return dict(G=Gw, R=R, ntiles=ntiles, slabs=_cdiv(maxlen, max(R // Gw, 1)) + 1, streamk=True)


def _last_cut(g):                          # fwd_sched / tap_sched (line 677)
    return (1 if (g.Ho - 1) * g.stride - g.pad + 2 > g.H - 1 else 0, 1 if (g.Wo - 1) * g.stride - g.pad + 2 > g.W - 1 else 0)


def _cnt2(h, q):                           # igemm.h ClassSched::cnt2
    return h + min(h >> 1, q - 1)


def cls_plan(g, direction, kc, opt):
    """the position-class schedule of a forward or data-gradient product (igemm.h ClassSched through fwd_sched / dgrad_sched)"""
    if direction == "fwd":
        gh, gw, ncols, cin = g.Ho, g.Wo, g.Co, g.C
        lsh, lsw = _last_cut(g)
        Ah, Bw, amax, bmax = 3 * gh - 1 - lsh, 3 * gw - 1 - lsw, (3 if gh > 2 else 3 - max(1, lsh)), (3 if gw > 2 else 3 - max(1, lsw))
        s2 = False
    else:
        gh, gw, ncols, cin = g.H, g.W, g.C, g.Co
        s2 = g.stride == 2
        if s2:
            Ah, Bw = _cnt2(gh, g.Ho), _cnt2(gw, g.Wo)
            amax, bmax = (2 if gh >= 2 and g.Ho >= 2 else 1), (2 if gw >= 2 and g.Wo >= 2 else 1)
        else:
            Ah, Bw, amax, bmax = 3 * gh - 2, 3 * gw - 2, (3 if gh > 2 else 2), (3 if gw > 2 else 2)
    MB, ntn, nchunk = _cdiv(g.N, 128), _cdiv(ncols, 128), cin // kc
    p = _pool(nchunk * ntn * Ah * Bw * MB, gh * gw * MB * ntn, amax * bmax * nchunk, opt)
    p.update(grid=(gh, gw), MB=MB, ntn=ntn, s2=s2, last_cut=_last_cut(g) if direction == "fwd" else (1, 1),
             ragged_cols=bool(ncols % 128), ragged_rows=bool(g.N % 128))
    return p


def tap_plan(g, opt):
    """the weight gradient by taps (igemm.h TapSched through tap_sched)"""
    lsh, lsw = _last_cut(g)
    kpp, tpt = _cdiv(g.N, 128) * 128 // 32, (g.C // 128) * _cdiv(g.Co, 128)
    nh = [g.Ho - 1, g.Ho, g.Ho - lsh]
    nw = [g.Wo - 1, g.Wo, g.Wo - lsw]
    lens = [nh[t // 3] * nw[t % 3] * kpp for t in range(9)]
    p = _pool(sum(lens) * tpt, 9 * tpt, max(lens), opt)
    p.update(grid=(g.Ho, g.Wo), last_cut=(lsh, lsw), ragged_cols=bool(g.Co % 128), ragged_rows=bool(g.N % 128))
    return p


def parity_classes(g):
    """trunk.hip dgrad_parity: (ph, pw, Hc, Wc, kh0, kw0, nkh, nkw) of the four classes of input positions"""
    out = []
    for ph in (0, 1):
        for pw in (0, 1):
            kh0, kw0 = (ph + g.pad) & 1, (pw + g.pad) & 1
            out.append((ph, pw, (g.H - ph + 1) // 2, (g.W - pw + 1) // 2, kh0, kw0,
                        (g.KS - kh0 + 1) // 2 if kh0 < g.KS else 0, (g.KS - kw0 + 1) // 2 if kw0 < g.KS else 0))
    return out


def conv_plan(direction, desc, b16=False, ws=True, accumulate=0, **opt):
    """What ``avvad_conv2d_<direction>[_bf16]`` launches for descriptor ``desc`` (a dict of DESC_FIELDS), restated from
    csrc/trunk.hip; ``ws``: a workspace of avvad_engine_workspace() bytes is given; ``opt``: the options of OPTIONS that are
    not at their defaults.  -> dict(form = one of FORMS or "REFUSED", tile, buf, streamk, adds = the extra additions of the
    rounding bound, ...)."""
    assert direction in DIRECTIONS and set(opt) <= set(OPTIONS), (direction, opt)
    g = geom(desc)
    if g is None:
        return dict(form="REFUSED", why="conv_geom")
    slab = bool(ws)
    if b16 and not _bf16_conv_ok(g):                                   # conv_fwd / conv_dgrad / conv_wgrad (lines 782, 880, 934)
        return dict(form="REFUSED", why="bf16_conv_ok")
    T = g.KS * g.KS
    refuse = lambda why: dict(form="REFUSED", why=why)                 # noqa: E731
    if direction == "fwd":                                             # fwd_form (lines 646-653)
        M, K, cols = g.N * g.Ho * g.Wo, T * g.C, (64 if g.Co <= 64 else 128)
        if _conv64_ok(g, b16, opt):
            grid = min(max(_cdiv(g.N * g.H * g.W, 32), 1), _grid_cus(opt))           # conv64.h grid_for (line 346)
            return dict(form="CONV64", grid=grid, tiles_per_wg=_cdiv(_cdiv(M, 32), grid), last_tile=M % 32, streamk=False, adds=0)
        if _fwd16_cls_ok(g, slab, opt) if b16 else _fwd_cls_ok(g, slab, opt):
            p = cls_plan(g, "fwd", 64 if b16 else 32, opt)
            return dict(p, form="CLS", adds=p["slabs"])
        if b16:
            p = engine_rounds(M, g.Co, K // 2, 128, cols, True, slab, 0, opt)
            return dict(p, form="ENGINE", buf=True, adds=p["slabs"])
        if g.Co % 4:                                                   # conv_fwd_engine (line 767)
            return refuse("Co % 4")
        if g.C == 1:                                                   # (line 652)
            if _stem_kernel_ok(g, opt):
                return dict(form="STEM", streamk=False, adds=0)
            p = engine_rounds(M, g.Co, K, 128, 64, False, slab, 0, opt)
            return dict(p, form="ENGINE", buf=False, stem=True, adds=p["slabs"])
        if g.C % 32 or not _taps_fit(g) or not (g.N * g.H * g.W * g.C < FITS_U30 and K * g.Co < FITS_U30):      # (line 773)
            return refuse("C % 32, Co % 4 or the tap mask")
        rows = 256 if g.Co <= 64 and not opt.get("no_tall", 0) else 128                                         # (line 653)
        buf = _fits_buf(g.N * g.H * g.W * g.C) and _fits_buf(T * g.C * g.Co) and not opt.get("no_buf", 0)
        p = engine_rounds(M, g.Co, K, rows, cols, False, slab, 0, opt)
        return dict(p, form="ENGINE", buf=buf, adds=p["slabs"])
    if direction == "dgrad":                                           # dgrad_form (lines 657-663)
        M, K, cols, acc = g.N * g.H * g.W, T * g.Co, (64 if g.C <= 64 else 128), 1 if accumulate else 0
        if _conv64_ok(g, b16, opt):
            grid = min(max(_cdiv(M, 32), 1), _grid_cus(opt))
            return dict(form="CONV64", grid=grid, tiles_per_wg=_cdiv(_cdiv(M, 32), grid), last_tile=M % 32, streamk=False, adds=acc)
        if _dgrad16_cls_ok(g, slab, opt) if b16 else _dgrad_cls_ok(g, slab, opt):
            p = cls_plan(g, "dgrad", 64 if b16 else 32, opt)
            return dict(p, form="CLS", adds=p["slabs"] + acc)
        buf = b16 or (_fits_buf(g.N * g.Ho * g.Wo * g.Co) and _fits_buf(T * g.C * g.Co) and not opt.get("no_buf", 0))
        if not b16 and (g.Co % 32 or g.C % 4 or not _taps_fit(g)):     # conv_dgrad_engine (line 854)
            return refuse("Co % 32, C % 4 or the tap mask")
        if g.stride == 2:                                              # (line 662) -> dgrad_parity (lines 833-836)
            live = [c for c in parity_classes(g) if g.N * c[2] * c[3] > 0 and c[6] * c[7] > 0]
            if any(c[6] * c[7] > 4 for c in live):
                return refuse("a parity class of more than 4 taps")
            ps = [engine_rounds(g.N * c[2] * c[3], g.C, c[6] * c[7] * g.Co // (2 if b16 else 1), 128, cols, b16, slab, 1, opt) for c in live]
            return dict(form="PARITY", tile=(128, cols), buf=buf, classes=[(c[0], c[1], c[6] * c[7]) for c in live],
                        dead=4 - len(live), streamk=any(p["streamk"] for p in ps), slabs=max(p["slabs"] for p in ps),
                        adds=max(p["slabs"] for p in ps) + 1)
        rows = 256 if cols == 64 and not b16 and not opt.get("no_tall", 0) else 128                             # (line 663)
        p = engine_rounds(M, g.C, K // (2 if b16 else 1), rows, cols, b16, slab, acc, opt)
        return dict(p, form="ENGINE", buf=buf, adds=p["slabs"] + acc)
    # wgrad_form (lines 665-670)
    M, K, cols = T * g.C, g.N * g.Ho * g.Wo, (64 if g.Co <= 64 else 128)
    if b16:
        if (K + 32) * (g.Ho * g.Wo) >= (1 << 32):
            return refuse("fast_div range")
        if _wgrad16_tap_ok(g, slab, opt):                              # (line 667)
            p = tap_plan(g, opt)
            return dict(p, form="TAP", adds=p["slabs"])
        p = engine_rounds(M, g.Co, K, 128, cols, True, slab, 0, opt)
        return dict(p, form="ENGINE", buf=True, adds=p["slabs"])
    if _conv64_wgrad_ok(g, slab, opt):
        grid = min(g.N * g.H, _grid_cus(opt))                          # (line 950)
        return dict(form="CONV64", grid=grid, rows_per_wg=_cdiv(g.N * g.H, grid), streamk=False, adds=grid)
    if _wgrad_tap_ok(g, slab, opt):
        p = tap_plan(g, opt)
        return dict(p, form="TAP", adds=p["slabs"])
    if g.Co % 4:                                                       # conv_wgrad_engine (line 910)
        return refuse("Co % 4")
    if g.C == 1:                                                       # (line 670)
        if _stem_wgrad_ok(g, slab, opt):
            nb = min(g.N, 256)                                         # (line 941)
            return dict(form="STEM", grid=nb, streamk=False, adds=nb)
        p = engine_rounds(M, g.Co, K, 64, 64, False, slab, 0, opt)
        return dict(p, form="ENGINE", buf=False, stem=True, adds=p["slabs"])
    if g.C % 32 or (K + 32) * (g.Ho * g.Wo) >= (1 << 32):              # (line 921)
        return refuse("C % 32 or the fast_div range")
    buf = _fits_buf(g.N * g.H * g.W * g.C) and _fits_buf(g.N * g.Ho * g.Wo * g.Co) and not opt.get("no_buf", 0)
    p = engine_rounds(M, g.Co, K, 128, cols, False, slab, 0, opt)
    return dict(p, form="ENGINE", buf=buf, adds=p["slabs"])


# ------------------------------------------------------------------------------------------ the cases
CASES = {}


def _case(name, N, Hh, W, C, Co, KS, stride, pad, forms, why="", path="f32", ws=1, acc=0, opts=None, tier="exact", reach=None):
    """``forms``: the kernel form each of fwd / dgrad / wgrad is meant to reach ("REFUSED": AVVAD_EINVAL; None: the direction is
    not run).  ``path``: "f32" the fp32 entry points, "opt" the same under option bf16 = 1, "b16" the _bf16 entry points.
    ``reach``: {direction: {field of conv_plan: value}} the case is there for."""
    opts = dict(opts or {})
    if path == "opt":
        opts["bf16"] = 1
    c = dict(d=dict(N=N, H=Hh, W=W, C=C, Co=Co, KS=KS, stride=stride, pad=pad), forms=dict(zip(DIRECTIONS, forms)), path=path,
             ws=ws, acc=acc, opts=opts, tier=tier, why=why, reach=reach or {})
    assert name not in CASES and path in ("f32", "opt", "b16") and tier in ("exact", "round"), name
    g = geom(c["d"])
    assert g is not None, name
    c["K"] = dict(fwd=KS * KS * C, dgrad=KS * KS * Co, wgrad=N * g.Ho * g.Wo)
    assert all(64 * k + 8 < 2 ** 24 for k in c["K"].values()), name      # the exact tier's condition (the rounding tier is smaller still)
    CASES[name] = c
    return name


def _c(n, **kw):
    return dict(max_cus=n, **kw)


E, P, RF = "ENGINE", "PARITY", "REFUSED"

# ---- ENGINE, fp32: KS 1 .. 5 x stride 1, 2 x pad {0, KS // 2, KS - 1} on a 7 x 5 image (H != W; pad = KS - 1: the output is
# larger than the input), C alternating 32 / 96, Co 64 / 160, accumulate alternating.  Stride 2 is the PARITY form (up to 4 taps
# per class: KS <= 4) and must be refused for KS = 5 BEFORE dx is cleared.
SWEEP = []
_i = 0
for _ks in (1, 2, 3, 4, 5):
    for _pad in sorted({0, _ks // 2, _ks - 1}):
        for _s in (1, 2):
            _C, _Co = (32, 160) if _i % 2 else (96, 64)
            _dg = E if _s == 1 else (P if _ks <= 4 else RF)
            SWEEP.append(_case("k%d-s%d-p%d" % (_ks, _s, _pad), 3, 7, 5, _C, _Co, _ks, _s, _pad, (E, _dg, E), acc=_i // 2 % 2))
            _i += 1

ENGINE = [
    _case("h1", 3, 1, 9, 32, 64, 3, 1, 1, (E, E, E), "H = 1"),
    _case("w1", 3, 9, 1, 32, 64, 3, 2, 1, (E, P, E), "W = 1, stride 2"),
    _case("ks5-h2", 2, 2, 6, 32, 32, 5, 1, 2, (E, E, E), "KS > H with padding", acc=1),
    _case("ks4-h3-p3", 2, 3, 4, 32, 32, 4, 2, 3, (E, P, E), "KS > H, pad = KS - 1, stride 2"),
    _case("co4", 5, 9, 7, 32, 4, 3, 1, 1, (E, RF, E), "Co = 4: one ragged 64-column tile; dgrad needs Co % 32 == 0"),
    _case("co36", 5, 9, 7, 32, 36, 3, 1, 1, (E, RF, E), "Co = 36"),
    _case("co68", 5, 9, 7, 32, 68, 3, 1, 1, (E, RF, E), "Co = 68: 128-column tiles, one ragged"),
    _case("co160-c96", 5, 9, 7, 96, 160, 3, 1, 1, (E, E, E), "Co = 160: two column tiles, the second ragged", acc=1),
    _case("tall", 3, 11, 9, 32, 64, 3, 1, 1, (E, E, E), "297 pixels on the 256 x 64 tall tile: two tiles, the second ragged",
          reach=dict(fwd=dict(tile=(256, 64), ntiles=2, ragged=True), dgrad=dict(tile=(256, 64)), wgrad=dict(tile=(128, 64)))),
    _case("tall-no_tall", 3, 11, 9, 32, 64, 3, 1, 1, (E, E, E), "the same on 128 x 64 tiles", opts=dict(no_tall=1),
          reach=dict(fwd=dict(tile=(128, 64), ntiles=3), dgrad=dict(tile=(128, 64)))),
    _case("tall-nows", 3, 11, 9, 32, 64, 3, 1, 1, (E, E, E), "no workspace: whole tiles", ws=0, acc=1,
          reach=dict(fwd=dict(streamk=False), wgrad=dict(streamk=False))),
]
# stream-K with split tiles on a capped grid: 572 pixels x 160 columns x K = 864 on 2 CUs (G = 4): 10 tiles = 2 full rounds and a
# pool of 2 tiles; the weight gradient 864 x 160 x K = 572: 14 tiles = 3 full rounds and a pool of 2
_SK = (4, 13, 11, 96, 160, 3, 1, 1)
_SKR = dict(fwd=dict(G=4, full_rounds=2, rem=2, streamk=True, tile=(128, 128)), wgrad=dict(G=4, full_rounds=3, rem=2, streamk=True))
ENGINE += [
    _case("sk", *_SK, (E, E, E), "stream-K, one-wave fix-up", opts=_c(2),
          reach=dict(_SKR, fwd=dict(_SKR["fwd"], fixup="fixup1", buf=True), dgrad=dict(streamk=True, tile=(128, 128)))),
    _case("sk-acc", *_SK, (None, E, None), "dgrad += on split tiles", opts=_c(2), acc=1, reach=dict(dgrad=dict(streamk=True))),
    _case("sk-no_fixup1", *_SK, (E, E, E), "the four-wave fix-up", opts=_c(2, no_fixup1=1), acc=1,
          reach=dict(fwd=dict(fixup="fixup"), wgrad=dict(fixup="fixup"))),
    _case("sk-no_streamk", *_SK, (E, E, E), "whole tiles by option", opts=_c(2, no_streamk=1),
          reach=dict(fwd=dict(streamk=False, full_rounds=3), wgrad=dict(streamk=False))),
    _case("sk-no_buf", *_SK, (E, E, E), "flat-addressed gathers", opts=_c(2, no_buf=1), acc=1,
          reach=dict(fwd=dict(buf=False, streamk=True), dgrad=dict(buf=False), wgrad=dict(buf=False))),
    _case("sk-nows", *_SK, (E, E, E), "no workspace", opts=_c(2), ws=0, reach=dict(fwd=dict(streamk=False))),
    _case("sk-c8", *_SK, (E, E, E), "8 CUs: every tile in the pool", opts=_c(8), reach=dict(fwd=dict(full_rounds=0, streamk=True))),
    _case("sk-bf16opt", *_SK, (E, E, E), "option bf16 = 1 on the fp32 entry points", path="opt", opts=_c(2), acc=1),
    _case("k2-s2-bf16opt", 3, 8, 7, 64, 64, 2, 2, 1, (E, P, E), "option bf16 = 1, even kernel, parity classes", path="opt"),
]

# ---- PARITY: the stride-2 data gradient below 128 images (forward and weight gradient ride along on the engine)
PARITY = [
    _case("par-k3-7x7", 3, 7, 7, 64, 32, 3, 2, 1, (E, P, E), "3x3 / pad 1: classes of 1 / 2 / 2 / 4 taps, odd x odd",
          reach=dict(dgrad=dict(classes=[(0, 0, 1), (0, 1, 2), (1, 0, 2), (1, 1, 4)]))),
    _case("par-k3-6x8", 3, 6, 8, 64, 32, 3, 2, 1, (E, P, E), "even x even", acc=1),
    _case("par-k3-7x6", 3, 7, 6, 32, 64, 3, 2, 1, (E, P, E), "odd x even"),
    _case("par-k3-6x7", 3, 6, 7, 32, 64, 3, 2, 1, (E, P, E), "even x odd", acc=1),
    _case("par-k1", 3, 7, 6, 64, 32, 1, 2, 0, (E, P, E), "1x1 / pad 0: three classes have no tap -- their dx must be zero",
          reach=dict(dgrad=dict(dead=3))),
    _case("par-k1-acc", 3, 6, 7, 64, 32, 1, 2, 0, (None, P, None), "... or the old value when accumulating", acc=1,
          reach=dict(dgrad=dict(dead=3))),
    _case("par-k2", 3, 7, 6, 32, 32, 2, 2, 0, (E, P, E), "2x2 / pad 0: every class has one tap"),
    _case("par-k2-p1", 3, 6, 7, 32, 32, 2, 2, 1, (E, P, E), "2x2 / pad 1", acc=1),
    _case("par-k4-p1", 3, 8, 7, 32, 32, 4, 2, 1, (E, P, E), "4x4 / pad 1: four taps in every class"),
    _case("par-k4-p1-acc", 2, 7, 8, 32, 32, 4, 2, 1, (None, P, None), acc=1),
    _case("par-sk", 7, 13, 11, 128, 64, 3, 2, 1, (None, P, None), "split tiles inside the class products", opts=_c(1),
          reach=dict(dgrad=dict(streamk=True))),
]

# ---- C == 1: the stem
ST = "STEM"
STEM = [
    _case("stem-9x12", 3, 9, 12, 1, 64, 7, 2, 3, (ST, RF, ST), "the LDS-resident kernels on a small frame (Wo = 6)"),
    _case("stem-12x9", 2, 12, 9, 1, 64, 7, 2, 3, (ST, RF, E), "an odd Wo = 5: the weight gradient falls back to the engine"),
    _case("stem-8x72", 2, 8, 72, 1, 64, 7, 2, 3, (ST, RF, E), "an even Wo = 36 > 34: falls back too"),
    _case("stem-8x68", 2, 8, 68, 1, 64, 7, 2, 3, (ST, RF, ST), "Wo = 34: the widest the kernel's register rows hold"),
    _case("stem-640x12", 1, 640, 12, 1, 64, 7, 2, 3, (ST, RF, ST), "646 x 19 floats: 49096 bytes of LDS, just inside the budget"),
    _case("stem-641x12", 1, 641, 12, 1, 64, 7, 2, 3, (E, RF, E), "647 x 19 floats: 49172 bytes, just over it",
          reach=dict(fwd=dict(stem=True))),
    _case("stem-9x12-no_stem", 3, 9, 12, 1, 64, 7, 2, 3, (E, RF, E), opts=dict(no_stem_kernel=1)),
    _case("stem-9x12-nows", 3, 9, 12, 1, 64, 7, 2, 3, (ST, None, E), "no workspace: no room for the partials", ws=0),
    _case("stem-co32", 2, 9, 12, 1, 32, 7, 2, 3, (E, RF, E), "Co = 32: the engine's StemFwd / StemWgradX"),
    _case("stem-co128", 2, 9, 12, 1, 128, 7, 2, 3, (E, RF, E), "Co = 128"),
    _case("stem-k3", 2, 8, 10, 1, 32, 3, 1, 1, (E, RF, E), "3x3 / 1 on one channel"),
    _case("stem-k5", 2, 8, 10, 1, 128, 5, 1, 2, (E, RF, E), "5x5 / 1 on one channel"),
    _case("stem-k5-c8", 40, 8, 10, 1, 128, 5, 1, 2, (E, RF, E), "... with split tiles", opts=_c(1),
          reach=dict(fwd=dict(streamk=True), wgrad=dict(streamk=True))),
]

# ---- CONV64: 64 -> 64 channels, 3x3 / 1 / 1
C64 = "CONV64"
CONV64 = [
    _case("c64-1px", 1, 1, 1, 64, 64, 3, 1, 1, (C64, C64, C64), "one pixel"),
    _case("c64-5x7", 1, 5, 7, 64, 64, 3, 1, 1, (C64, C64, C64), "35 pixels: a last tile of 3", reach=dict(fwd=dict(last_tile=3))),
    _case("c64-h1", 2, 1, 9, 64, 64, 3, 1, 1, (C64, C64, C64), "H = 1", acc=1),
    _case("c64-w18", 2, 3, 18, 64, 64, 3, 1, 1, (C64, C64, C64), "W = 18: the widest row of the weight-gradient kernel"),
    _case("c64-w19", 2, 3, 19, 64, 64, 3, 1, 1, (C64, C64, E), "W = 19: the weight gradient leaves it, the forward stays", acc=1),
    _case("c64-c2", 6, 9, 13, 64, 64, 3, 1, 1, (C64, C64, C64), "22 tiles on 2 workgroups: the cross-tile prefetch, 2 partials", opts=_c(2),
          reach=dict(fwd=dict(grid=2, tiles_per_wg=11, last_tile=30), wgrad=dict(grid=2, rows_per_wg=27))),
    _case("c64-c2-acc", 6, 9, 13, 64, 64, 3, 1, 1, (None, C64, None), "dgrad +=", opts=_c(2), acc=1),
    _case("c64-c7", 5, 7, 6, 64, 64, 3, 1, 1, (C64, C64, C64), "7 workgroups: 7 tiles, one of 18 pixels; 35 rows", opts=_c(7)),
    _case("c64-no_conv64", 6, 9, 13, 64, 64, 3, 1, 1, (E, E, E), "the engine on the same problem", opts=dict(no_conv64=1), acc=1,
          reach=dict(fwd=dict(tile=(256, 64)))),
    _case("c64-nows", 2, 5, 7, 64, 64, 3, 1, 1, (C64, C64, E), "no workspace: the weight gradient has no room for partials", ws=0),
    _case("c64-b16", 6, 9, 13, 64, 64, 3, 1, 1, (C64, C64, E), "the bf16 form", path="b16", opts=_c(2)),
    _case("c64-b16-acc", 2, 5, 7, 64, 64, 3, 1, 1, (C64, C64, E), "the bf16 form, dgrad +=", path="b16", acc=1),
    _case("c64-bf16opt", 2, 5, 7, 64, 64, 3, 1, 1, (E, E, E), "option bf16 = 1 leaves the fp32 form", path="opt"),
]

# ---- CLS and TAP: 3x3 / pad 1 from 128 images up
CL, TP = "CLS", "TAP"
CLS = [
    _case("cls-2x2", 128, 2, 2, 128, 128, 3, 1, 1, (CL, CL, TP), "a 2x2 grid: every position loses a tap row and a tap column",
          reach=dict(fwd=dict(grid=(2, 2), ntiles=4), wgrad=dict(ntiles=9))),
    _case("cls-2x3", 129, 2, 3, 128, 160, 3, 1, 1, (CL, CL, TP), "2x3, 129 images (a second image block of one row), ragged columns",
          acc=1, reach=dict(fwd=dict(ragged_cols=True, ragged_rows=True, MB=2))),
    _case("cls-3x2", 257, 3, 2, 160, 128, 3, 1, 1, (CL, CL, E), "3x2, 257 images, C = 160: dgrad with ragged columns, wgrad on the engine",
          reach=dict(dgrad=dict(ragged_cols=True, MB=3))),
    _case("cls-3x3", 128, 3, 3, 256, 256, 3, 1, 1, (CL, CL, TP), "3x3", acc=1),
    _case("cls-5x4", 129, 5, 4, 128, 256, 3, 1, 1, (CL, CL, TP), "5x4"),
    _case("cls-s2-5x6", 128, 5, 6, 128, 128, 3, 2, 1, (CL, CL, TP), "stride 2, H odd and W even: a 3x3 grid whose last column loses no tap",
          reach=dict(fwd=dict(grid=(3, 3), last_cut=(1, 0)), dgrad=dict(s2=True, grid=(5, 6)), wgrad=dict(last_cut=(1, 0)))),
    _case("cls-s2-6x5", 129, 6, 5, 128, 256, 3, 2, 1, (CL, CL, TP), "stride 2, H even and W odd", acc=1,
          reach=dict(fwd=dict(last_cut=(0, 1)))),
    _case("cls-s2-4x4", 128, 4, 4, 256, 128, 3, 2, 1, (CL, CL, TP), "stride 2, even x even: a 2x2 grid whose last row and column lose no tap",
          reach=dict(fwd=dict(grid=(2, 2), last_cut=(0, 0)))),
    _case("cls-s2-7x7", 128, 7, 7, 128, 128, 3, 2, 1, (CL, CL, TP), "stride 2, odd x odd: a 4x4 grid", acc=1,
          reach=dict(fwd=dict(grid=(4, 4), last_cut=(1, 1)))),
    _case("cls-s2-4x6", 257, 4, 6, 128, 160, 3, 2, 1, (CL, CL, TP), "stride 2: a 2x3 grid, 257 images, ragged columns"),
    _case("cls-s2-no_s2_cls", 128, 5, 6, 128, 128, 3, 2, 1, (CL, P, TP), "the four parity launches at N >= 128", opts=dict(no_s2_cls=1)),
    _case("cls-no_cls", 128, 3, 3, 256, 256, 3, 1, 1, (E, E, E), "the engine on the same problem", opts=dict(no_cls=1), acc=1),
    _case("cls-cap4", 128, 2, 2, 128, 128, 3, 1, 1, (CL, CL, E), "cls_cap = 4: the 4 class tiles fit, the 9 tap tiles do not", opts=dict(cls_cap=4)),
    _case("cls-cap3", 128, 2, 2, 128, 128, 3, 1, 1, (E, E, E), "cls_cap = 3: one below the class products' tile count", opts=dict(cls_cap=3)),
    _case("cls-cap9", 128, 2, 2, 128, 128, 3, 1, 1, (CL, CL, TP), "cls_cap = 9: the tap tiles just fit", opts=dict(cls_cap=9), acc=1),
    _case("cls-c2", 128, 2, 2, 128, 128, 3, 1, 1, (CL, CL, E), "2 CUs: a cap of 8 tiles, 4 workers", opts=_c(2),
          reach=dict(fwd=dict(G=4))),
    _case("cls-ho1", 128, 1, 3, 128, 128, 3, 1, 1, (E, E, E), "Ho = 1 leaves the class forms"),
    _case("cls-n127", 127, 3, 3, 128, 128, 3, 1, 1, (E, E, E), "127 images: one below the class forms"),
]

# ---- the bf16 data path (_bf16 entry points)
B16 = [
    _case("b16-co128", 3, 9, 7, 64, 128, 3, 1, 1, (E, E, E), "128 x 128 tiles", path="b16", reach=dict(fwd=dict(tile=(128, 128)))),
    _case("b16-co64", 3, 9, 7, 128, 64, 3, 1, 1, (E, E, E), "128 x 64 tiles (forward, weight gradient)", path="b16", acc=1,
          reach=dict(fwd=dict(tile=(128, 64)), dgrad=dict(tile=(128, 128)))),
    _case("b16-sk", 4, 13, 11, 128, 192, 3, 1, 1, (E, E, E), "stream-K with split tiles", path="b16", opts=_c(2), acc=1,
          reach=dict(fwd=dict(streamk=True))),
    _case("b16-nows", 4, 13, 11, 128, 192, 3, 1, 1, (E, E, E), "no workspace", path="b16", opts=_c(2), ws=0,
          reach=dict(fwd=dict(streamk=False))),
    _case("b16-cls", 128, 3, 3, 128, 128, 3, 1, 1, (CL, CL, TP), "class forward (Ho Wo <= 9, Co >= 128), class dgrad, taps", path="b16"),
    _case("b16-cls-acc", 129, 2, 3, 128, 256, 3, 1, 1, (CL, CL, TP), "2x3, 129 images, dgrad +=", path="b16", acc=1),
    _case("b16-s2cls", 128, 7, 6, 128, 128, 3, 2, 1, (E, CL, E), "the stride-2 class data gradient on a 7x6 grid", path="b16",
          reach=dict(dgrad=dict(s2=True, grid=(7, 6)))),
    _case("b16-co64-cls", 128, 3, 3, 128, 64, 3, 1, 1, (E, CL, E), "Co = 64: no class forward, no taps", path="b16", acc=1),
    _case("b16-par", 3, 7, 6, 64, 128, 3, 2, 1, (E, P, E), "parity classes", path="b16"),
    _case("b16-par-k1", 3, 7, 6, 64, 128, 1, 2, 0, (E, P, E), "1x1 / 2 downsample", path="b16", acc=1),
    _case("b16-k2-s2", 3, 8, 7, 64, 64, 2, 2, 1, (E, P, E), "an even kernel, stride 2, pad 1", path="b16"),
    _case("b16-k4-p3", 3, 5, 7, 64, 128, 4, 1, 3, (E, E, E), "4x4 / pad 3: the output is larger than the input", path="b16", acc=1),
    _case("b16-k5-p2", 3, 7, 5, 128, 64, 5, 1, 2, (E, E, E), "5x5 / pad 2", path="b16"),
]

# ---- refusals that are decided by the shape alone (the launchers' guards cited in CITES)
REFUSALS = [
    _case("ref-c48", 2, 5, 5, 48, 64, 3, 1, 1, (RF, None, RF), "C % 32 != 0"),
    _case("ref-co6", 2, 5, 5, 32, 6, 3, 1, 1, (RF, RF, RF), "Co % 4 != 0: the weight gradient's 16-byte fetches of dy would run past it"),
    _case("ref-stem-co6", 2, 9, 12, 1, 6, 7, 2, 3, (RF, RF, RF), "Co % 4 != 0 on one channel"),
    _case("ref-k7-c32", 2, 9, 9, 32, 64, 7, 1, 3, (RF, RF, None), "49 taps do not fit the 32-bit tap mask"),
    _case("ref-b16-c32", 2, 5, 5, 32, 64, 3, 1, 1, (RF, RF, RF), "bf16: C = 32", path="b16"),
    _case("ref-b16-co96", 2, 5, 5, 64, 96, 3, 1, 1, (RF, RF, RF), "bf16: Co = 96", path="b16"),
    _case("ref-k5-s2", 2, 9, 9, 32, 32, 5, 2, 2, (None, RF, None), "stride 2 with KS = 5: a parity class of 9 taps -- refused BEFORE dx is cleared"),
    _case("ref-b16-k5-s2", 2, 9, 9, 64, 64, 5, 2, 2, (None, RF, None), "the same on the bf16 path", path="b16"),
]

# ---- the rounding tier
ROUNDING = [
    _case("round-sk", *_SK, (E, E, E), opts=_c(2), acc=1, tier="round"),
    _case("round-sk-no_fixup1", *_SK, (E, E, E), opts=_c(2, no_fixup1=1), tier="round"),
    _case("round-k5-p4", 3, 7, 5, 32, 64, 5, 1, 4, (E, E, E), tier="round"),
    _case("round-par-k4", 3, 8, 7, 32, 32, 4, 2, 1, (E, P, E), acc=1, tier="round"),
    _case("round-stem", 3, 9, 12, 1, 64, 7, 2, 3, (ST, None, ST), tier="round"),
    _case("round-c64", 6, 9, 13, 64, 64, 3, 1, 1, (C64, C64, C64), opts=_c(2), acc=1, tier="round"),
    _case("round-cls", 129, 3, 3, 128, 160, 3, 1, 1, (CL, CL, TP), acc=1, tier="round"),
    _case("round-cls-s2", 128, 5, 6, 128, 128, 3, 2, 1, (CL, CL, TP), tier="round"),
    _case("round-sk-bf16opt", *_SK, (E, E, E), path="opt", opts=_c(2), tier="round"),
    _case("round-b16-sk", 4, 13, 11, 128, 192, 3, 1, 1, (E, E, E), path="b16", opts=_c(2), acc=1, tier="round"),
    _case("round-b16-cls", 128, 3, 3, 128, 128, 3, 1, 1, (CL, CL, TP), path="b16", tier="round"),
    _case("round-b16-c64", 6, 9, 13, 64, 64, 3, 1, 1, (C64, C64, E), path="b16", opts=_c(2), acc=1, tier="round"),
    _case("round-b16-par", 3, 7, 6, 64, 128, 3, 2, 1, (E, P, E), path="b16", tier="round"),
]
GROUPS = ("SWEEP", "ENGINE", "PARITY", "STEM", "CONV64", "CLS", "B16", "REFUSALS", "ROUNDING")


def plan_of(name, direction):
    c = CASES[name]
    return conv_plan(direction, c["d"], b16=c["path"] == "b16", ws=bool(c["ws"]), accumulate=c["acc"], **c["opts"])


# ------------------------------------------------------------------------------------------ buffers and reference
def _to_bf16(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).bfloat16().float().numpy()


def _draw(rng, tier, *shape):
    if tier == "exact":
        return rng.integers(-8, 9, shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


@functools.lru_cache(maxsize=4)
def _inputs(name):
    """the logical operands of a case (float32): x NCHW, w OIHW, dy NCHW, dx0 NCHW"""
    c = CASES[name]
    g = geom(c["d"])
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x, w = _draw(rng, c["tier"], g.N, g.C, g.H, g.W), _draw(rng, c["tier"], g.Co, g.C, g.KS, g.KS)
    dy, dx0 = _draw(rng, c["tier"], g.N, g.Co, g.Ho, g.Wo), _draw(rng, c["tier"], g.N, g.C, g.H, g.W)
    if c["tier"] == "round" and c["path"] != "f32":
        x, w, dy = _to_bf16(x), _to_bf16(w), _to_bf16(dy)               # value-pinned: what the bf16 operands hold
    return x, w, dy, dx0


def _nhwc(t):
    return np.ascontiguousarray(np.transpose(t, (0, 2, 3, 1)))


def pack_f32(w):
    """avvad_conv2d_pack_weights: wf[(kh, kw, c)][co], wd[(kh, kw, co)][c] from w OIHW"""
    Co, C, KS, _ = w.shape
    return (np.ascontiguousarray(np.transpose(w, (2, 3, 1, 0))).reshape(KS * KS * C, Co),
            np.ascontiguousarray(np.transpose(w, (2, 3, 0, 1))).reshape(KS * KS * Co, C))


def pack_bf16_index(Co, C, KS):
    """avvad_conv2d_pack_weights_bf16: for every element of w OIHW, its place in wf16[co][(c >> 6, tap, c & 63)] and in
    wd16[c][(co >> 6, tap, co & 63)]"""
    T = KS * KS
    co, c, tap = np.meshgrid(np.arange(Co), np.arange(C), np.arange(T), indexing="ij")
    return (co * (T * C) + ((c >> 6) * T + tap) * 64 + (c & 63)).reshape(-1), (c * (T * Co) + ((co >> 6) * T + tap) * 64 + (co & 63)).reshape(-1)


@functools.lru_cache(maxsize=4)
def reference(name):
    """{direction: (ref, S)} in float64 in the ABI's layouts: y NHWC, dx NHWC (dx0 + dgrad when the case accumulates),
    dw[(kh, kw, c)][co]; S: the same sums of absolute values"""
    import torch
    import torch.nn.functional as F
    c = CASES[name]
    g = geom(c["d"])
    x, w, dy, dx0 = (torch.from_numpy(t).double() for t in _inputs(name))
    out = {}

    def run(x, w, dy):
        x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y = F.conv2d(x, w, None, g.stride, g.pad)
        y.backward(dy)
        return y.detach().numpy(), x.grad.numpy(), w.grad.numpy()
    (y, dx, dw), (ya, dxa, dwa) = run(x, w, dy), run(x.abs(), w.abs(), dy.abs())
    if c["acc"]:
        dx, dxa = dx + dx0.numpy(), dxa + dx0.abs().numpy()
    out["fwd"] = (_nhwc(y), _nhwc(ya))
    out["dgrad"] = (_nhwc(dx), _nhwc(dxa))
    perm = lambda t: np.ascontiguousarray(np.transpose(t, (2, 3, 1, 0))).reshape(g.KS * g.KS * g.C, g.Co)      # noqa: E731
    out["wgrad"] = (perm(dw), perm(dwa))
    return out


def _guarded(X, fill):
    buf = np.full(GUARD + X.size + GUARD, fill, dtype=np.float32)
    buf[GUARD:GUARD + X.size] = X.reshape(-1)
    return buf


OUT_BUF = dict(fwd="y_buf", dgrad="dx_buf", wgrad="dw_buf")


def prepare(name):
    """fresh buffers of a case, each [GUARD][logical][GUARD] floats: x_buf, dy_buf, w_buf (OIHW), wf_buf, wd_buf with NaN guards;
    y_buf and dw_buf NaN inside -0.0 guards, dx_buf = dx0 inside -0.0 guards.  (The bf16 paths' operands are these values, which
    bf16 holds exactly; the GPU test narrows them on the way to the device.)"""
    c = CASES[name]
    g = geom(c["d"])
    x, w, dy, dx0 = _inputs(name)
    wf, wd = pack_f32(w)
    minus0 = np.float32(-0.0)
    b = types.SimpleNamespace(name=name, case=c, g=g, d=c["d"], ws=bool(c["ws"]), acc=c["acc"], path=c["path"],
                              x_buf=_guarded(_nhwc(x), np.nan), dy_buf=_guarded(_nhwc(dy), np.nan), w_buf=_guarded(w, np.nan),
                              wf_buf=_guarded(wf, np.nan), wd_buf=_guarded(wd, np.nan),
                              y_buf=_guarded(np.full((g.N, g.Ho, g.Wo, g.Co), np.nan, np.float32), minus0),
                              dx_buf=_guarded(_nhwc(dx0), minus0),
                              dw_buf=_guarded(np.full((g.KS * g.KS * g.C, g.Co), np.nan, np.float32), minus0))
    return b


def view(bufs, what):
    """the logical part of a buffer in the ABI's layout"""
    g = bufs.g
    shape = dict(x_buf=(g.N, g.H, g.W, g.C), dx_buf=(g.N, g.H, g.W, g.C), dy_buf=(g.N, g.Ho, g.Wo, g.Co), y_buf=(g.N, g.Ho, g.Wo, g.Co),
                 dw_buf=(g.KS * g.KS * g.C, g.Co), wf_buf=(g.KS * g.KS * g.C, g.Co), wd_buf=(g.KS * g.KS * g.Co, g.C))[what]
    buf = getattr(bufs, what)
    return buf[GUARD:buf.size - GUARD].reshape(shape)


def bound_factor(name, direction):
    """(K + A + 8) 2^-24 of the rounding tier"""
    p = plan_of(name, direction)
    return (CASES[name]["K"][direction] + p["adds"] + 8) * 2.0 ** -24


def scaled_error(name, direction, bufs):
    ref, S = reference(name)[direction]
    got = view(bufs, OUT_BUF[direction]).astype(np.float64)
    bound = bound_factor(name, direction) * S
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / bound, np.where(err == 0, 0.0, 1e30))


def check_conv(impl, name, tag="gpu"):
    """``impl(bufs, direction) -> rc`` runs one direction on ``bufs`` (see ``prepare``).  Before anything is launched the restated
    plan must give the form the case names, and what it is listed to reach.  Then per direction: rc; every float of the output
    buffer outside the logical part keeps the sentinel's bits; a refusal leaves EVERY bit; exact tier: the result EQUALS the
    float64 reference cast to float32; rounding tier: |got - ref| <= (K + A + 8) 2^-24 S element-wise.  Returns the worst
    error / bound over the directions (0 for the exact tier)."""
    c = CASES[name]
    plans = {}
    for direction in DIRECTIONS:
        want = c["forms"][direction]
        if want is None:
            continue
        p = plans[direction] = plan_of(name, direction)
        assert p["form"] == want, "%s %s: the plan says %s, the case list %s" % (name, direction, p["form"], want)
        for k, v in c["reach"].get(direction, {}).items():
            assert p[k] == v, "%s %s: %s is %r, the case list says %r" % (name, direction, k, p[k], v)
    bufs = prepare(name)
    refs = reference(name)
    worst = 0.0
    for direction, p in plans.items():
        out = getattr(bufs, OUT_BUF[direction])
        before = out.view(np.uint32).copy()
        rc = impl(bufs, direction)
        bits = out.view(np.uint32)
        if p["form"] == "REFUSED":
            assert rc == EINVAL, "%s %s: returned %r, not AVVAD_EINVAL (%s)" % (name, direction, rc, p["why"])
            bad = np.flatnonzero(bits != before)
            assert bad.size == 0, "%s %s: refused, but %d floats of the output buffer changed, the first at %d" % (
                name, direction, bad.size, bad[0] - GUARD)
            continue
        assert rc == 0, "%s %s: returned %r" % (name, direction, rc)
        for lo, hi, what in ((0, GUARD, "in front of"), (out.size - GUARD, out.size, "behind")):
            bad = np.flatnonzero(bits[lo:hi] != SENTINEL)
            assert bad.size == 0, "%s %s: %d floats of the guard %s the output were written, the first at %d" % (
                name, direction, bad.size, what, bad[0] + lo - GUARD)
        ref, S = refs[direction]
        got = view(bufs, OUT_BUF[direction]).astype(np.float64)
        assert got.shape == ref.shape
        nf = np.argwhere(~np.isfinite(got))
        assert nf.size == 0, "%s %s (%s): %d non-finite elements (an element nobody wrote, or a guard multiplied in), the first at %s" % (
            name, direction, p["form"], len(nf), tuple(nf[0]))
        if c["tier"] == "exact":
            assert float(np.abs(ref).max(initial=0.0)) < 2 ** 24 and np.array_equal(ref, np.round(ref))
            wrong = np.argwhere(got != ref)
            assert wrong.size == 0, "%s %s (%s): %d of %d elements differ from the exact result; the first at %s: got %r, exact %r; " \
                "index ranges %s .. %s" % (name, direction, p["form"], len(wrong), got.size, tuple(wrong[0]), got[tuple(wrong[0])],
                                           ref[tuple(wrong[0])], wrong.min(axis=0).tolist(), wrong.max(axis=0).tolist())
            continue
        scaled = scaled_error(name, direction, bufs)
        ratio = H.report(FAMILY, "%s %s |d| / ((K + %d + 8) 2^-24 S)" % (name, direction, p["adds"]), scaled, np.zeros_like(scaled),
                         1.0, tag=tag)
        worst = max(worst, ratio)
    return worst


# ------------------------------------------------------------------------------------------ the float32 CPU twin
MUTANTS = ("tap_dropped", "kernel_not_flipped", "parity_neighbour", "padding_live", "ragged_row_dropped", "dx_ignored", "dx_twice",
           "class_row_shifted", "dw_ckk_order")


def _fwd_index(g, live_padding=False):
    """[Ho Wo][T] -> input pixel hi W + wi of tap (kh, kw) at output pixel (ho, wo); H W where the tap is in the padding"""
    ho, wo, kh, kw = np.meshgrid(np.arange(g.Ho), np.arange(g.Wo), np.arange(g.KS), np.arange(g.KS), indexing="ij")
    hi, wi = ho * g.stride - g.pad + kh, wo * g.stride - g.pad + kw
    ok = (hi >= 0) & (hi < g.H) & (wi >= 0) & (wi < g.W)
    if live_padding:
        hi, wi, ok = np.clip(hi, 0, g.H - 1), np.clip(wi, 0, g.W - 1), np.ones_like(ok)
    return np.where(ok, hi * g.W + wi, g.H * g.W).reshape(g.Ho * g.Wo, g.KS * g.KS)


def _dgrad_index(g, mutant=None):
    """[H W][T] -> output pixel of tap (kh, kw) at input pixel (hi, wi): ho = (hi + pad - kh) / stride where that is whole and
    inside dy; Ho Wo otherwise"""
    hi, wi, kh, kw = np.meshgrid(np.arange(g.H), np.arange(g.W), np.arange(g.KS), np.arange(g.KS), indexing="ij")
    if mutant == "kernel_not_flipped":
        kh, kw = g.KS - 1 - kh, g.KS - 1 - kw
    hq, wq = hi + g.pad - kh, wi + g.pad - kw
    if mutant == "parity_neighbour":                  # the row's class takes the taps of the class next to it
        ok = ((hq + 1) % g.stride == 0) & (wq % g.stride == 0)
        hq = hq + 1
    else:
        ok = (hq % g.stride == 0) & (wq % g.stride == 0)
    ho, wo = hq // g.stride, wq // g.stride
    ok = ok & (ho >= 0) & (ho < g.Ho) & (wo >= 0) & (wo < g.Wo)
    if mutant == "padding_live":
        ok = (hq % g.stride == 0) & (wq % g.stride == 0)
        ho, wo = np.clip(ho, 0, g.Ho - 1), np.clip(wo, 0, g.Wo - 1)
    return np.where(ok, ho * g.Wo + wo, g.Ho * g.Wo).reshape(g.H * g.W, g.KS * g.KS)


def _images(buf, N, per, shift):
    """the N images of ``per`` floats each; ``shift`` = 1: image n is image n + 1, and the last one is what lies behind the
    operand (NaN, as the guard)"""
    imgs = buf[GUARD:GUARD + N * per].reshape(N, per)
    return imgs if not shift else np.concatenate([imgs[1:], np.full((1, per), np.nan, np.float32)])


def twin(bufs, direction, mutant=None):
    """float32 evaluation on the prepared buffers: a plain im2col and one float32 product per direction.  ``mutant``: one of
    MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    g, f32 = bufs.g, np.float32
    p = plan_of(bufs.name, direction)
    if p["form"] == "REFUSED":
        return EINVAL
    T = g.KS * g.KS
    shift = 1 if (mutant == "class_row_shifted" and p["form"] in ("CLS", "TAP")) else 0
    if mutant == "class_row_shifted" and not shift:
        raise ValueError("mutant class_row_shifted needs a class form")
    tile_rows = p["tile"][0] if "tile" in p else (32 if p["form"] == "CONV64" else 128)
    if direction == "fwd":
        x = _images(bufs.x_buf, g.N, g.H * g.W * g.C, shift).reshape(g.N, g.H * g.W, g.C)
        x = np.concatenate([x, np.zeros((g.N, 1, g.C), f32)], axis=1)
        cols = x[:, _fwd_index(g, mutant == "padding_live")]                      # [N][Ho Wo][T][C]
        if mutant == "tap_dropped":
            cols[:, :, T - 1] = 0
        y = (cols.reshape(g.N * g.Ho * g.Wo, T * g.C) @ view(bufs, "wf_buf")).astype(f32)
        out = view(bufs, "y_buf").reshape(g.N * g.Ho * g.Wo, g.Co)
        rows = y.shape[0] - (1 if mutant == "ragged_row_dropped" else 0)
        if mutant == "ragged_row_dropped" and y.shape[0] % tile_rows == 0:
            raise ValueError("mutant ragged_row_dropped needs a ragged tile")
        out[:rows] = y[:rows]
    elif direction == "dgrad":
        dy = _images(bufs.dy_buf, g.N, g.Ho * g.Wo * g.Co, shift).reshape(g.N, g.Ho * g.Wo, g.Co)
        dy = np.concatenate([dy, np.zeros((g.N, 1, g.Co), f32)], axis=1)
        cols = dy[:, _dgrad_index(g, mutant)]                                     # [N][H W][T][Co]
        if mutant == "tap_dropped":
            cols[:, :, T - 1] = 0
        dx = (cols.reshape(g.N * g.H * g.W, T * g.Co) @ view(bufs, "wd_buf")).astype(f32)
        out = view(bufs, "dx_buf").reshape(g.N * g.H * g.W, g.C)
        if mutant in ("dx_ignored", "dx_twice") and not bufs.acc:
            raise ValueError("mutant %s needs an accumulating case" % mutant)
        if bufs.acc and mutant != "dx_ignored":
            dx = (out + dx).astype(f32)
            if mutant == "dx_twice":
                dx = (dx + out).astype(f32)
        rows = dx.shape[0]
        out[:rows] = dx[:rows]
    else:
        x = _images(bufs.x_buf, g.N, g.H * g.W * g.C, shift).reshape(g.N, g.H * g.W, g.C)
        x = np.concatenate([x, np.zeros((g.N, 1, g.C), f32)], axis=1)
        cols = x[:, _fwd_index(g, mutant == "padding_live")]                      # [N][Ho Wo][T][C]
        if mutant == "tap_dropped":
            cols[:, :, T - 1] = 0
        a = cols.reshape(g.N * g.Ho * g.Wo, T, g.C)
        a = np.transpose(a, (2, 1, 0) if mutant == "dw_ckk_order" else (1, 2, 0))     # rows (kh kw, c) -- the mutant's: (c, kh kw)
        dw = (a.reshape(T * g.C, g.N * g.Ho * g.Wo) @ view(bufs, "dy_buf").reshape(g.N * g.Ho * g.Wo, g.Co)).astype(f32)
        out = view(bufs, "dw_buf")
        rows = dw.shape[0]
        out[:rows] = dw[:rows]
    return 0


def log_worst(tag):
    H.log_worst(tag)
