"""The oracle of the encoder tests: a float64 restatement of the WaveNet encoder (``oracle.wavenet.encode``) with explicit
ReLU masks, the case list, and ONE assertion function, ``check_encoder``.  It takes the implementation under test as a
callable: tests/test_encoder_gpu.py passes the HIP path (csrc/wavenet.hip), tests/test_encoder_cpu.py passes the float32 CPU
oracle (the bounds must be within reach of a correct float32 evaluation) and mutants of it (every assertion must be able to
fail).

Why the masks are explicit.  The encoder has three families of ReLU units -- ``s`` (the input of block i), ``z`` (the
dilation output of block i) and ``b`` (the bottleneck output) -- and the kernels never store a pre-activation, so a test
cannot look up on which side of zero the implementation put a unit.  A unit whose float64 pre-activation is within rounding
of zero may legitimately land on either side in float32, and its gradient path is then switched the other way: a finite
difference in every upstream gradient.  The suite's older answer is a relative-L2 alternative that is always open.  Here:

* the reference's ReLU is ``x * mask`` with ``mask = (x > 0)``, XORed at an explicit list ``flips`` of units;
* ``ambiguous(case)`` is the list of units with ``|pre64| < TAU``, ascending in ``|pre64|``;
* ``check_encoder`` compares every gradient element-wise with the reference under its own masks; only if that fails does it
  look for a set S of at most ``MAX_FLIPS`` = 3 units of ``ambiguous(case)`` (greedy, ascending ``|pre|``, one float64
  backward per trial), and the verdict is the same strict element-wise comparison against ``reference(case, flips=S)`` -- an
  exact evaluation of the same network with those units on the other side.  There is no aggregate alternative anywhere.

TAU = 8e-6.  Measured by tests/test_encoder_cpu.py: over the case list the float32 oracle's pre-activations are within
9.9e-8 (T3) .. 8.1e-7 (E4, the 20-block stack) of the float64 ones and no ReLU decision differs, so TAU is 9.9 x the worst
spread; the test asserts the factor 8.  (8 = a second valid float32 order -- MFMA's chain against the host's vector sums,
each within 1 x of exact -- and 4 x head-room.)  The cases have 0 .. 88 ambiguous units (T6: 88, E9: 62, E4: 49, E3: 22), cap 128.

Bounds.  Outputs: 2e-5 max(1, max|ref|) (what test_wavenet_block_kernel_forms_agree holds one block to against float64).
Gradients: 1e-4 max(1, max|ref|) element-wise.  The float32 CPU oracle meets both at a ratio <= 0.25 with 0 flips in every
case (asserted by the CPU test; measured: outputs <= 0.033, gradients <= 0.070).  The float32 stand-in runs on ONE thread:
with several, the CPU library sums the bottleneck's bias gradient over E9's 16 568 samples in an order that is itself
0.2 .. 2.3 x the bound off (30 seeds, 2 .. 16 threads), which says something about that sum and nothing about the bound; on
one thread the same 30 seeds give 0.05 .. 0.44, the case's own 0.06.  Every comparison goes through ``head_ref.report`` with family "enc": error, bound and ratio
go to the parity log."""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

import head_ref as H
from oracle import wavenet as ow

FAMILY = "enc"
TAU = 8e-6
MAX_FLIPS = 3
MAX_AMBIGUOUS = 128
UPSTREAM = 3.0                # factor on the loss before backward()
OUT_BOUND = 2e-5              # x max(1, max|ref|)
RUNS = []                     # (tag, label, flips) of every check_encoder run that passed

W0_DIL = [2 ** i for i in range(10)] * 2

# B, L, dilations, Bn, P; R = D = 32, fw = 2, qc = 1, biases on unless stated.  Lv: samples in front of the pool.  What each
# case reaches is asserted by tests/test_encoder_cpu.py against the restated form choices below.
CASES = {
    # Lv = 32: exactly one tile per layer end / 33: one tile + one sample; tail forward <1>, tail backward MFMA
    "E1": dict(B=1, L=40, dil=[1, 2, 4], Bn=32, P=4, seed=1),
    "E1r": dict(B=1, L=41, dil=[1, 2, 4], Bn=32, P=4, seed=2),
    # a tap that crosses tiles (64), an odd dilation, ragged last tiles in every layer, odd row pitches, overlapping pool
    # bins (197 / 7), tail PAIR
    "E2": dict(B=2, L=300, dil=[1, 2, 64, 3, 32], Bn=256, P=7, seed=3),
    # 140 tiles per layer: the fused backward's grid 9 -> 8 (rounded down), the forward's 35 -> 40 (surplus waves), several
    # tiles per wave
    "E3": dict(B=7, L=700, dil=[64, 3], Bn=256, P=7, seed=4),
    # full depth, dilation 512, Lv = 103
    "E4": dict(B=2, L=2150, dil=W0_DIL, Bn=256, P=9, seed=5),
    # B > 32: narrow_conv1d_grads wraps its 32 sequence groups; Bn % 128 != 0
    "E5": dict(B=33, L=150, dil=[1, 32], Bn=64, P=4, seed=6),
    # every generic kernel, engine weight gradients; n: null bias pointers
    "E6": dict(B=3, L=120, dil=[1, 2, 5], Bn=40, P=5, R=16, D=24, fw=3, qc=2, seed=7),
    "E6n": dict(B=3, L=120, dil=[1, 2, 5], Bn=40, P=5, R=16, D=24, fw=3, qc=2, bias=False, seed=8),
    # MFMA blocks with the GENERIC tail
    "E7": dict(B=2, L=100, dil=[1, 2], Bn=48, P=3, seed=9),
    # tail_fwd_mfma<4> with the unfused MFMA tail backward
    "E8": dict(B=2, L=100, dil=[4], Bn=128, P=3, seed=10),
    # Lo >= 8192: the dwordx4 forward, with a tap offset that is no multiple of 4
    "E9": dict(B=2, L=8800, dil=[512, 3], Bn=32, P=6, seed=115),
    # P > Lv: a sample lies in more than two bins.  Lv = 3 < P = 5 at the Bn of PAIR / MFMA / GENERIC (all three take the
    # generic tail backward since its loop walks the full range)
    "T1-256": dict(B=2, L=6, dil=[1, 1], Bn=256, P=5, seed=12),
    "T1-32": dict(B=2, L=6, dil=[1, 1], Bn=32, P=5, seed=13),
    "T1-48": dict(B=2, L=6, dil=[1, 1], Bn=48, P=5, seed=14),
    # W0's P = 60 with Lv = 53
    "T2": dict(B=1, L=69, dil=[1, 2, 4, 8], Bn=256, P=60, seed=15),
    # Lv = 1: the one sample is in every bin
    "T3": dict(B=2, L=5, dil=[1, 2], Bn=32, P=4, seed=16),
    # P = Lv (every bin one sample), P = 1 (one bin)
    "T4": dict(B=2, L=40, dil=[1, 2, 4], Bn=32, P=32, seed=17),
    "T5": dict(B=2, L=40, dil=[1, 2, 4], Bn=32, P=1, seed=18),
    # 1026 time tiles in front of the fused tail backward, more than its 4 x TAIL_MAXBLK waves (pairs): the pair form's second
    # round (2 live pairs of 1024, the rest dead between workgroup barriers), the one-wave form's second stride step, the slab
    # reduce over all 256 slabs.  Lv = 33: one full tile + a one-sample tile per sequence, overlapping bins
    "T6": dict(B=513, L=35, dil=[1], Bn=256, P=4, seed=21),
}


def config(name):
    c = CASES[name]
    return dict(filter_width=c.get("fw", 2), quantization_channel=c.get("qc", 1), dilations=list(c["dil"]),
                en_residual_channel=c.get("R", 32), en_dilation_channel=c.get("D", 32), en_bottleneck_width=c["Bn"],
                en_pool_kernel_size=c["P"], use_bias=c.get("bias", True))


def lengths(name):
    """[L_0 (behind the causal layer), L_1, ..., L_N = Lv]"""
    c = CASES[name]
    fw = c.get("fw", 2)
    Ls = [c["L"] - (fw - 1)]
    for d in c["dil"]:
        Ls.append(Ls[-1] - d * (fw - 1))
    return Ls


@functools.lru_cache(maxsize=None)
def inputs(name):
    """float32: wave uniform in (-1, 1), parameters from ``oracle.wavenet.init_params``, a normal cotangent G"""
    c, cfg = CASES[name], config(name)
    gen = torch.Generator().manual_seed(c["seed"])
    params = ow.init_params(cfg, generator=gen)
    wave = torch.rand(c["B"], cfg["quantization_channel"], c["L"], generator=gen) * 2 - 1
    G = torch.randn(c["B"], c["Bn"], c["P"], generator=gen)
    return types.SimpleNamespace(name=name, cfg=cfg, params=params, wave=wave, G=G)


# ------------------------------------------------------------------------------------------ the restatement
def pool_bins(Lv, P):
    """AdaptiveAvgPool1d(P) over Lv samples: bin p is [floor(p Lv / P), ceil((p + 1) Lv / P))"""
    return [((p * Lv) // P, -((-(p + 1) * Lv) // P)) for p in range(P)]


def pool_matrix(Lv, P, dtype, form="exact"):
    """M (P, Lv) with out = s @ M^T.  ``exact``: M[p][t] = 1 / len_p inside bin p.  ``end_rounded_down``: the bin end as
    floor((p + 1) Lv / P).  ``three_bin_window``: bin p reaches sample t only if |p - floor(t P / Lv)| <= 1, which is how
    the tail-backward kernels looked the bins up before P > Lv was sent to the full range."""
    M = torch.zeros(P, Lv, dtype=dtype)
    for p, (a, e) in enumerate(pool_bins(Lv, P)):
        if form == "end_rounded_down":
            e = ((p + 1) * Lv) // P
        M[p, a:e] = 1.0 / max(e - a, 1)
    if form == "three_bin_window":
        c0 = (torch.arange(Lv) * P) // Lv
        M = M * ((torch.arange(P)[:, None] - c0[None, :]).abs() <= 1).to(dtype)
    return M


def _mix(value, grad_path):
    """the value of ``value`` (exactly: x + (y - y)) with the gradient of ``grad_path``: a backward that is wrong behind a
    forward that is right"""
    return value.detach() + (grad_path - grad_path.detach())


MUTANTS = ("taps_swapped", "residual_wrong_end", "wgrad_drops_last_tile", "bgrad_drops_last_sample",
           "causal_ignores_seq_32", "pool_end_rounded_down", "pool_three_bin_window")


def encode_restated(params, wave, cfg, flips=(), mutant=None, grad_only_flips=False, block=1):
    """``oracle.wavenet.encode`` with the ReLU as ``x * mask``: -> (out, pre), pre[(family, i)] the pre-activations of
    ("s", i) the input of block i, ("z", i) its dilation output, ("b", 0) the bottleneck output.  ``flips``: units
    (family, i, b, channel, t) whose mask is inverted (``grad_only_flips``: in the backward only).  ``mutant``: one of
    ``MUTANTS``, a BACKWARD that is wrong in block ``block`` (or the causal layer / the pool) behind an unchanged forward."""
    assert mutant is None or mutant in MUTANTS, mutant
    g = params.get
    pre = {}

    def relu(x, fam, i):
        pre[(fam, i)] = x
        mask = x.detach() > 0
        y = x * mask.to(x.dtype)
        here = [u for u in flips if (u[0], u[1]) == (fam, i)]
        if here:
            m2 = mask.clone()
            for _, _, b, c, t in here:
                m2[b, c, t] = ~m2[b, c, t]
            y2 = x * m2.to(x.dtype)
            y = _mix(y, y2) if grad_only_flips else y2
        return y

    cw, cb = params["en_causal_layer.weight"], g("en_causal_layer.bias")
    s = F.conv1d(wave, cw, cb)
    if mutant == "causal_ignores_seq_32":            # the parameter gradients of the causal layer stop at sequence 31
        live = (torch.arange(wave.shape[0]) < 32).to(s.dtype)[:, None, None]
        wd = wave.detach()
        full = F.conv1d(wd, cw, cb)
        s = F.conv1d(wave, cw.detach(), None if cb is None else cb.detach()) + live * (full - full.detach())
    for i, d in enumerate(cfg["dilations"]):
        cur = s
        w1, b1 = params["en_dilation_layer_stack.%d.weight" % i], g("en_dilation_layer_stack.%d.bias" % i)
        w2, b2 = params["en_dense_layer_stack.%d.weight" % i], g("en_dense_layer_stack.%d.bias" % i)
        x = relu(s, "s", i)
        z = F.conv1d(x, w1, b1, dilation=d)
        m = mutant if i == block else None
        if m == "taps_swapped":
            z = _mix(z, F.conv1d(x, w1.flip(-1), b1, dilation=d))
        elif m == "wgrad_drops_last_tile":           # d W_dil without the last 32-sample tile of the last sequence
            Lo = z.shape[2]
            live = torch.ones(z.shape[0], 1, Lo, dtype=z.dtype)
            live[-1, :, ((Lo - 1) // 32) * 32:] = 0
            part = F.conv1d(x.detach(), w1, None, dilation=d)
            z = F.conv1d(x, w1.detach(), b1, dilation=d) + live * (part - part.detach())
        y = F.conv1d(relu(z, "z", i), w2, b2)
        if m == "bgrad_drops_last_sample" and b2 is not None:     # d b_dense without the last sample of the last sequence
            live = torch.ones_like(y)
            live[-1, :, -1] = 0
            y = _mix(y, F.conv1d(relu(z, "z", i), w2, None) + live * b2[None, :, None])
        n = y.shape[2]
        res = cur[:, :, -n:]
        if m == "residual_wrong_end":
            res = _mix(res, cur[:, :, :n])
        s = y + res
    zb = F.conv1d(s, params["bottleneck_layer.weight"], g("bottleneck_layer.bias"))
    a = relu(zb, "b", 0)
    P = cfg["en_pool_kernel_size"]
    out = F.adaptive_avg_pool1d(a, P)
    if mutant in ("pool_end_rounded_down", "pool_three_bin_window"):
        out = _mix(out, a @ pool_matrix(a.shape[2], P, a.dtype, mutant[5:]).t())
    return out, pre


def run(name, dtype, flips=(), frozen=(), mutant=None, grad_only_flips=False, keep_pre=False, passes=1):
    """forward + backward of UPSTREAM * sum(out * G) in ``dtype``: -> namespace(out, grads, pre).  grads maps "wave" and
    every parameter name to its gradient, None for what ``frozen`` names."""
    inp = inputs(name)
    params = {k: v.to(dtype).clone().requires_grad_(k not in frozen) for k, v in inp.params.items()}
    wave = inp.wave.to(dtype).clone().requires_grad_("wave" not in frozen)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                  # (see the module docstring: the float32 stand-in and the thread count)
    try:
        for _ in range(passes):
            out, pre = encode_restated(params, wave, inp.cfg, flips, mutant, grad_only_flips)
            ((out * inp.G.to(dtype)).sum() * UPSTREAM).backward()
    finally:
        torch.set_num_threads(threads)
    grads = {k: v.grad for k, v in params.items()}
    grads["wave"] = wave.grad
    return types.SimpleNamespace(out=out.detach(), grads=grads, pre={k: v.detach() for k, v in pre.items()} if keep_pre else None)


@functools.lru_cache(maxsize=None)
def _reference0(name):
    return run(name, torch.float64, keep_pre=True)


def reference(name, flips=()):
    """the float64 evaluation with the units ``flips`` on the other side of their ReLU (cached without flips)"""
    flips = tuple(flips)
    return _reference0(name) if not flips else run(name, torch.float64, flips=flips)


def encoder_fp32(inp, frozen=(), flips=(), mutant=None, grad_only_flips=False, passes=1):
    """the float32 CPU stand-in: the restatement in float32 (bit for bit ``oracle.wavenet.encode`` without a mutant)"""
    r = run(inp.name, torch.float32, flips=flips, frozen=frozen, mutant=mutant, grad_only_flips=grad_only_flips, passes=passes)
    return dict(out=r.out, grads=r.grads)


@functools.lru_cache(maxsize=None)
def ambiguous(name):
    """the units (family, i, b, channel, t) with |pre64| < TAU, ascending in |pre64|"""
    units = []
    for (fam, i), x in _reference0(name).pre.items():
        for b, c, t in (x.abs() < TAU).nonzero().tolist():
            units.append((abs(float(x[b, c, t])), (fam, i, b, c, t)))
    return tuple(u for _, u in sorted(units))


# ------------------------------------------------------------------------------------------ the assertion
def _errors(got, ref, scale, keys):
    """per tensor: (worst |got - scale ref| / bound, flat index of that element); and the sum of squared ratios, the score
    of the flip search"""
    worst, score = {}, 0.0
    for k in keys:
        r = ref[k].double() * scale
        ratio = (got[k].detach().cpu().double() - r).abs() / (1e-4 * max(1.0, float(r.abs().max())))
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
        i = int(ratio.argmax())
        worst[k] = (float(ratio.reshape(-1)[i]), i)
        score += float((ratio.clamp(max=1e6) ** 2).sum())
    return worst, score


def find_flips(got, name, scale, keys):
    """greedy, ascending |pre|: a unit of ``ambiguous(name)`` joins S if the float64 gradients with it flipped are closer
    (sum of squared error / bound over all compared tensors) to ``got``; at most MAX_FLIPS units.  -> (S, gradients)"""
    S, ref = [], reference(name).grads
    _, score = _errors(got, ref, scale, keys)
    for u in ambiguous(name):
        if len(S) == MAX_FLIPS:
            break
        trial = reference(name, S + [u]).grads
        _, sc = _errors(got, trial, scale, keys)
        if sc < score:
            S, ref, score = S + [u], trial, sc
    return tuple(S), ref


def check_encoder(impl, name, frozen=(), tag="gpu", label="", passes=1):
    """``impl(inp, frozen)`` -> dict(out, grads): out (B, Bn, P) and the gradients of UPSTREAM * sum(out * inp.G) after
    ``passes`` forward + backward passes without zeroing, grads["wave"] and grads[<parameter name>], None for what ``frozen``
    names.  Step 1: out.  Step 2: every gradient element-wise against ``passes`` x the float64 reference under its own masks.
    Step 3, only if step 2 fails: the same comparison against the reference with at most MAX_FLIPS units of
    ``ambiguous(name)`` flipped.  -> the flipped units."""
    inp = inputs(name)
    ref = reference(name)
    got = impl(inp, tuple(frozen))
    t = "%s%s%s " % (name, " " + label if label else "", " [frozen: %s]" % ",".join(frozen) if frozen else "")
    H.report(FAMILY, t + "out", got["out"], ref.out, OUT_BOUND * max(1.0, float(ref.out.abs().max())), tag=tag)
    grads = got["grads"]
    assert set(grads) == set(ref.grads), (sorted(grads), sorted(ref.grads))
    keys = []
    for k in sorted(ref.grads):
        if k in frozen:
            assert grads[k] is None, t + k + " is frozen and has a gradient"
        else:
            assert grads[k] is not None, t + k + " has no gradient"
            assert tuple(grads[k].shape) == tuple(ref.grads[k].shape), (k, grads[k].shape)
            keys.append(k)
    scale = float(passes)
    worst, _ = _errors(grads, ref.grads, scale, keys)
    S, ref_g = (), ref.grads
    if max(w for w, _ in worst.values()) > 1.0:
        S, ref_g = find_flips(grads, name, scale, keys)
        worst, _ = _errors(grads, ref_g, scale, keys)
        if tag is not None:
            H.log_line("head %-5s %-8s %sflip search: S = %s of %d ambiguous units" % (tag, FAMILY, t, list(S), len(ambiguous(name))))
    failed = []
    for k in keys:
        try:
            H.report_grad(FAMILY, t + "d/d" + k, grads[k], ref_g[k] * scale, tag=tag)
        except AssertionError as e:
            failed.append((worst[k][0], k, str(e)))
    if failed:
        ratio, k, msg = max(failed)
        idx = tuple(int(v) for v in np.unravel_index(worst[k][1], tuple(ref_g[k].shape)))
        raise AssertionError("%sd/d%s: element %s is %.3f x its bound (reference with flips S = %s; %d of %d gradients fail)\n%s"
                             % (t, k, idx, ratio, list(S), len(failed), len(keys), msg))
    assert len(S) <= MAX_FLIPS and set(S) <= set(ambiguous(name))
    if tag is not None:
        RUNS.append((tag, t.strip(), S))
    return S


def log_worst(tag):
    """the worst error / bound this process has seen for ``tag`` in family "enc", and how many runs needed a flip"""
    for (tg, family), (ratio, name) in sorted(H.WORST.items()):
        if tg == tag and family == FAMILY:
            H.log_line("head %-5s %-8s WORST ratio=%.4f  (%s)" % (tag, family, ratio, name))
    runs = [r for r in RUNS if r[0] == tag]
    flipped = [r for r in runs if r[2]]
    H.log_line("head %-5s %-8s runs: %d, of which %d needed a flip%s" % (
        tag, FAMILY, len(runs), len(flipped), "".join("; %s: %s" % (r[1], list(r[2])) for r in flipped)))


# ------------------------------------------------------------------------------------------ the form choices, restated
# csrc/wavenet.hip: wn_grid_size, fwd_form, dx_form, bwd_form, tail_fwd_form, tail_bwd_form under the default options (and
# wn_grid).
def cdiv(a, b):
    return -(-a // b)


def wn_grid_size(tiles, per_wg, cap, wn_grid, rnd):
    g = min(cdiv(tiles, per_wg), cap)
    if wn_grid > 0:
        g = min(g, wn_grid)
    if rnd == "up" or (rnd == "up_from_8" and g >= 8):
        g = cdiv(g, 8) * 8
    if rnd == "down_from_8" and g >= 8:
        g = g // 8 * 8
    return max(g, 1)


def fwd_form(B, Lin, dil, wn_flat=0, wn_grid=0):
    Lo = Lin - dil
    if wn_flat in (0, 3) and Lo >= 128 and (Lo >= 8192 or wn_flat == 3):
        return "WIDE", wn_grid_size(B * cdiv(Lo, 128), 4, wn_grid if wn_grid > 0 else 1024, 0, "up")
    tiles = B * cdiv(Lo, 32)
    if wn_flat == 5 and Lo >= 32:
        return "DMA", wn_grid_size(tiles, 8, 512, wn_grid, "up_from_8")
    if wn_flat in (0, 4):
        return "OCC", wn_grid_size(tiles, 4, 1024, wn_grid, "up_from_8")
    return ("FLAT" if wn_flat == 1 else "BUF"), wn_grid_size(tiles, 4, 512, wn_grid, "none")


def dx_form(B, Lin, wn_dx=0, wn_flat=0):
    tiles = B * cdiv(Lin, 32)
    if wn_flat != 1 and wn_dx in (0, 2):
        return "OCC", wn_grid_size(tiles, 4, 1024, 0, "up_from_8")
    return ("BUF" if wn_flat != 1 and wn_dx != 3 else "FLAT"), wn_grid_size(tiles, 4, 512, 0, "none")


def bwd_form(B, Lo, any_grad=True, wn_bwd_t=0, wn_no_fused_wgrad=0):
    tiles = B * cdiv(Lo, 32)
    if not any_grad or wn_no_fused_wgrad:
        return "UNFUSED", wn_grid_size(tiles, 16, 512, 0, "none")
    t = wn_bwd_t or 2
    if t == 3:
        return "RESIDENT", wn_grid_size(tiles, 16, 256, 0, "none")
    if t == 2:
        return "OCC", wn_grid_size(tiles, 16, 512, 0, "down_from_8")
    return "TRANSPOSED", wn_grid_size(tiles, 16, 512, 0, "none")


TAIL_MAXBLK = 256             # workgroups = slabs of the fused tail backward, four time tiles each per round


def tail_fwd_form(B, R, Bn, P):
    if not (R == 32 and Bn % 32 == 0):
        return "GENERIC", 0
    nt = 4 if Bn % 128 == 0 else 1
    return "<%d>" % nt, wn_grid_size(B * P * (Bn // (32 * nt)), 4, 2048, 0, "none")


def tail_bwd_form(Lv, R, Bn, P, any_grad=True, wn_no_fused_tail=0, wn_no_tail_pair=0):
    if not (R == 32 and Bn % 32 == 0 and Bn <= 1024) or P > Lv:
        return "GENERIC"
    if Bn == 256 and any_grad and not wn_no_fused_tail:
        return "FUSED" if wn_no_tail_pair else "PAIR"
    return "MFMA"


def mfma_shape(name):
    c = CASES[name]
    return c.get("R", 32) == 32 and c.get("D", 32) == 32 and c.get("fw", 2) == 2
