"""The oracle of the whole-trunk tests: a float64 restatement of the ResNet-18 trunk (``oracle.resnet18.trunk_forward``) whose
discrete decisions -- the 17 ReLU sign patterns and the max pool's window positions -- are ARGUMENTS, the case list, the form
choices of csrc/trunk.hip restated, and ONE assertion function, ``check_trunk``.  It takes the implementation under test as
a callable: tests/test_trunk_gpu.py passes the HIP path, tests/test_trunk_cpu.py passes the float32 CPU evaluation (the
bounds must be within reach of a correct float32 evaluation) and mutants of it (every assertion must be able to fail).

Why the decisions are arguments.  At N >= 128 a correct float32 evaluation of the trunk always puts a few of its 10 .. 30
million ReLU units on the other side of zero than float64 does (their pre-activations are within rounding of zero), and
each such unit moves every upstream gradient by a finite amount: 134 .. 680 x the element-wise bound.  The older tests
answer with a relative-L2 alternative, which then IS the verdict and hides an error of a few 1e-3 (one wrong grid position,
one class row).  The trunk keeps its post-ReLU activations and the pool's arg-max plane for its backward, so here:

* the implementation reports its own decisions (sign patterns, window positions), read before its backward;
* the DECISION RULE: a ReLU unit of layer k may differ from float64's only if |pre64| <= TAU[case][k]; a pool window may
  take another position only if float64's maximum exceeds the value there by at most TAU[case]["pool"]; and all differing
  decisions together are at most 2 + units // 1 000 000 per run (the cap ``test_gpu_parity._relu_flips`` uses).  A
  differing decision outside the rule fails with layer, index and |pre64|;
* VALUES are compared element-wise, with no aggregate alternative anywhere, against the float64 evaluation UNDER THE
  IMPLEMENTATION'S DECISIONS -- an exact evaluation of the network the implementation actually ran: features
  2e-5 max(1, max|ref|), each of the 60 gradients 1e-4 max(1, max|ref|), running statistics 1e-5 + 1e-5 |ref|.  (The
  reference under float64's own decisions is cached; it is re-evaluated once, 1 .. 2.5 s, only when a decision differs.
  The rule is checked on the pre-activations of the evaluation the values are compared with.)

TAU.  TAU[case][k] = 10 x the largest |pre32 - pre64| of the float32 CPU evaluation on layer k of that case, measured by
tests/test_trunk_cpu.py (which asserts the factor: at least 8, at most 16) and recorded below.  8 = a second valid float32
order (MFMA's chain against the host's vector sums, each within 1 x of exact) and 4 x head-room; 10 leaves the host's
thread count some room.  Spreads run from ~4e-6 at the stem to ~3e-5 at the last block in training mode, and to ~1.2e-4 in
eval mode, where the seeded running statistics let activations reach 260.

Measured.  Decisions that differ from float64 per run: float32 CPU evaluation 0 .. 4 ReLU units (caps 2 .. 25), MI355X 0 .. 10
(default options: T1 4, T1e 3, T2 3, T3 2, T4 0, T5 4, T6 9, T7 0, T7e 0, T8 8; T8 under no_streamk 10 of 25), all inside
the rule; no pool position differed anywhere.  Worst error / bound, MI355X | float32 CPU: features 0.21 | 0.15, gradients
0.070 | 0.069, running statistics 0.043 | 0.026.  (units counts the 17 saved tensors, as _relu_flips does: 8.4 M for
130 x 35x43, cap 10.)"""
import functools
import types

import torch
import torch.nn.functional as F

import head_ref as H
import stategen
from oracle import resnet18

FAMILY = "trunk"
FEAT_BOUND = 2e-5             # x max(1, max|ref|)
MOMENTUM, EPS = 0.1, 1e-5
RUNS = []                     # (tag, label, differing ReLU decisions, differing pool positions, cap) of every run that passed

NAMES = ["pool"] + ["%d.%d%s" % (4 + s, b, a) for s in range(4) for b in range(2) for a in (".a1", "")]   # the 17 layers

# N, H, W, training; the grid chains (stem, pool / layer1, layer2, layer3, layer4) are in the comments.  What each case
# reaches is asserted by tests/test_trunk_cpu.py against the restated form choices below.
CASES = {
    # 18x22, 9x11, 5x6, 3x3, 2x2: two class-row tiles, the second with 2 live rows; fused statistics through the CLS epilogue
    # and the fix-up; stride-2 class dgrad on an even width (6 -> 3); 5.0.conv1: CLS forward, PARITY dgrad, ENGINE wgrad
    "T1": dict(N=130, H=35, W=43, training=True, seed=101),
    "T1e": dict(N=130, H=35, W=43, training=False, seed=101),   # running statistics as scale / shift; coef k1 = k2 = 0
    # 26x18, 13x9, 7x5, 4x3, 2x2: whole class tiles, H > W, an even 4 -> 2 stride-2 step
    "T2": dict(N=128, H=51, W=35, training=True, seed=102),
    # as T1, one below the threshold: ENGINE / PARITY everywhere with ragged 128- and 256-row tiles
    "T3": dict(N=127, H=35, W=43, training=True, seed=103),
    # 16x16, 8x8, 4x4, 2x2, 1x1: the smallest frame; last stage 1x1 (CLS refused) beside CLS in layers 2, 3; avgpool HW = 1
    "T4": dict(N=130, H=32, W=32, training=True, seed=104),
    # 18x38, 9x19, 5x10, 3x5, 2x3: stem forward on the LDS kernel but its wgrad on the engine (Wo = 38 > 34); conv64 forward /
    # dgrad but wgrad on the engine (W = 19 > WG_MAXW); one live row in the second class tile
    "T5": dict(N=129, H=35, W=75, training=True, seed=105),
    # 18x18, 9x9, 5x5, 3x3, 2x2: three class-row tiles, the last with one row; stem_pool_relu_bwd's grid capped at 2048
    "T6": dict(N=257, H=35, W=35, training=True, seed=106),
    # 17x20, 9x10, 5x5, 3x3, 2x2: an odd stem height (the last pool window cut short) at the small-N forms
    "T7": dict(N=6, H=33, W=40, training=True, seed=107),
    "T7e": dict(N=6, H=33, W=40, training=False, seed=107),
    # 34, 17, 9, 5, 3: the workload's geometry with a ragged class tile
    "T8": dict(N=131, H=67, W=67, training=True, seed=108),
}

# 10 x the measured float32 spread per layer, in the order of NAMES (tests/test_trunk_cpu.py::test_tau_table)
TAU = {
    "T1": (4.0e-05, 4.9e-05, 6.3e-05, 5.7e-05, 8.9e-05, 7.1e-05, 1.2e-04, 1.2e-04, 1.5e-04, 1.4e-04, 1.7e-04, 1.5e-04, 2.2e-04, 1.5e-04, 1.9e-04, 1.7e-04, 2.5e-04),
    "T1e": (5.9e-05, 9.6e-05, 9.9e-05, 1.6e-04, 1.6e-04, 2.6e-04, 3.2e-04, 5.0e-04, 5.0e-04, 7.4e-04, 8.5e-04, 7.3e-04, 1.1e-03, 9.2e-04, 1.1e-03, 1.1e-03, 1.2e-03),
    "T2": (3.7e-05, 6.5e-05, 6.8e-05, 6.2e-05, 8.9e-05, 7.6e-05, 1.2e-04, 1.0e-04, 1.5e-04, 1.1e-04, 1.6e-04, 1.5e-04, 2.2e-04, 1.4e-04, 2.0e-04, 2.0e-04, 2.4e-04),
    "T3": (3.5e-05, 5.0e-05, 7.0e-05, 5.9e-05, 9.7e-05, 7.2e-05, 1.2e-04, 1.2e-04, 1.6e-04, 1.2e-04, 1.7e-04, 1.4e-04, 2.1e-04, 1.4e-04, 2.4e-04, 2.3e-04, 2.7e-04),
    "T4": (3.4e-05, 5.5e-05, 6.8e-05, 5.7e-05, 8.5e-05, 6.2e-05, 1.1e-04, 8.7e-05, 1.3e-04, 1.0e-04, 1.5e-04, 1.1e-04, 1.9e-04, 1.3e-04, 2.4e-04, 1.9e-04, 2.8e-04),
    "T5": (4.2e-05, 5.1e-05, 6.8e-05, 6.3e-05, 9.7e-05, 7.2e-05, 1.3e-04, 9.8e-05, 1.6e-04, 1.3e-04, 1.7e-04, 1.4e-04, 2.3e-04, 1.6e-04, 2.3e-04, 1.9e-04, 2.9e-04),
    "T6": (3.7e-05, 5.9e-05, 6.1e-05, 5.9e-05, 1.0e-04, 7.9e-05, 1.2e-04, 9.8e-05, 1.5e-04, 1.3e-04, 1.7e-04, 1.3e-04, 2.0e-04, 1.6e-04, 2.3e-04, 2.3e-04, 2.8e-04),
    "T7": (2.5e-05, 3.8e-05, 5.5e-05, 5.0e-05, 7.2e-05, 6.8e-05, 8.7e-05, 6.7e-05, 1.1e-04, 1.1e-04, 1.2e-04, 9.5e-05, 1.4e-04, 1.2e-04, 1.9e-04, 1.3e-04, 2.0e-04),
    "T7e": (3.5e-05, 6.9e-05, 7.2e-05, 1.3e-04, 1.3e-04, 2.3e-04, 3.0e-04, 3.1e-04, 4.1e-04, 6.2e-04, 5.8e-04, 6.5e-04, 7.4e-04, 6.7e-04, 1.1e-03, 9.8e-04, 1.1e-03),
    "T8": (5.4e-05, 5.6e-05, 7.2e-05, 6.4e-05, 1.3e-04, 7.1e-05, 1.2e-04, 1.2e-04, 1.6e-04, 1.2e-04, 2.1e-04, 1.7e-04, 2.5e-04, 2.3e-04, 2.8e-04, 2.3e-04, 3.5e-04),
}


def tau(case):
    return dict(zip(NAMES, TAU[case]))


# gradient subsets: what is frozen (keys without the "features." prefix)
def param_keys():
    return [k[len("features."):] for k, _ in resnet18.trunk_keys("features.") if k.rsplit(".", 1)[-1] in ("weight", "bias")]


def _is_conv(k):
    return k == "0.weight" or ".conv" in k or k.endswith("downsample.0.weight")


SUBSETS = {
    "stem_frozen": lambda k: k in ("0.weight", "1.weight", "1.bias"),       # the stem backward is skipped entirely
    "convs_frozen": _is_conv,                                                # BatchNorm trained
    "bn_frozen": lambda k: not _is_conv(k),                                  # convolutions trained
    "only_7_1": lambda k: not k.startswith("7.1."),
}


def frozen_keys(subset):
    return tuple(k for k in param_keys() if SUBSETS[subset](k))


@functools.lru_cache(maxsize=None)
def state():
    """the ``features.*`` entries of test_gpu_parity._video_state() (seed 7; the trunk's keys come first in its spec), keys
    without the prefix"""
    sd = stategen.make_state(resnet18.trunk_keys("features."), 7)
    return {k[len("features."):]: v for k, v in sd.items()}


@functools.lru_cache(maxsize=4)
def inputs(case):
    c = CASES[case]
    x = stategen.rand(c["seed"], c["N"], c["H"], c["W"])
    G = stategen.rand(c["seed"] + 1000, c["N"], 512)
    return types.SimpleNamespace(case=case, N=c["N"], H=c["H"], W=c["W"], training=c["training"], sd=state(), x=x, G=G)


def prefill(key, shape):
    """what ``accumulate`` puts into .grad before the backward"""
    return stategen.rand(5000 + param_keys().index(key), *shape)


# ------------------------------------------------------------------------------------------ the restatement
def _mix(value, grad_path):
    """the value of ``value`` with the gradient of ``grad_path``: a backward that is wrong behind a forward that is right"""
    return value.detach() + (grad_path - grad_path.detach())


class _MaskedBy(torch.autograd.Function):
    """z * fmask forward; the backward multiplies by box[0], filled in later (mutant a1_mask_from_output)"""

    @staticmethod
    def forward(ctx, z, fmask, box):
        ctx.box = box
        return z * fmask

    @staticmethod
    def backward(ctx, g):
        return g * ctx.box[0].to(g.dtype), None, None


def pool_windows(y, pad_value):
    """y (N,C,Hc,Wc) -> (9,N,C,Hp,Wp): the 3x3 / 2 / pad 1 windows, position dh*3+dw first; ``pad_value`` outside the image"""
    Hc, Wc = y.shape[2:]
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    yp = F.pad(y, (1, 2 * Wp + 1 - Wc - 1, 1, 2 * Hp + 1 - Hc - 1), value=pad_value)
    return torch.stack([yp[:, :, dh:dh + 2 * Hp:2, dw:dw + 2 * Wp:2] for dh in range(3) for dw in range(3)])


MUTANTS = ("pool_second_best", "pool_hw_swapped", "pool_drops_last", "stats_skip_rows_128", "stats_count_padded",
           "bn_bwd_no_mean_term", "running_var_biased", "a1_mask_from_output", "identity_before_ds_bn",
           "s2_dgrad_misses_last", "wgrad_short_of_last_image")


def trunk_restated(sd, x, training, masks=None, argmax=None, mutant=None):
    """``oracle.resnet18.trunk_forward`` on gray frames x (N,H,W) with every ReLU as ``z * mask`` and the pool as a gather.
    sd: keys without prefix.  masks: name -> bool (N,C,H,W) for the 17 layers of NAMES; argmax: (N,64,Hp,Wp) window
    positions dh*3+dw.  Left out, they are this evaluation's own: z > 0 and the first maximum in scan order.
    -> namespace(feat, stats (updated running statistics, sd untouched), pre (the 17 pre-activations; "pool": the largest
    pre-activation of the window), z0 (the stem's pre-activation), masks, argmax)."""
    assert mutant is None or mutant in MUTANTS, mutant
    dt = x.dtype
    N = x.shape[0]
    stats, pre, used = {}, {}, {}

    def bn(c, p, biased_running=False, skip=False, count_padded=False, no_mean_term=False):
        w, b, rm, rv = sd[p + ".weight"], sd[p + ".bias"], sd[p + ".running_mean"], sd[p + ".running_var"]
        if not training:
            stats[p + ".running_mean"], stats[p + ".running_var"] = rm.detach().clone(), rv.detach().clone()
            return (c - rm[None, :, None, None]) * (w / torch.sqrt(rv + EPS))[None, :, None, None] + b[None, :, None, None]
        src = c[:128] if skip else c
        n = src.numel() // src.shape[1]
        if count_padded:
            n = -(-N // 128) * 128 * c.shape[2] * c.shape[3]
        mean = src.sum((0, 2, 3)) / n
        var = (src * src).sum((0, 2, 3)) / n - mean * mean if count_padded else ((src - mean[None, :, None, None]) ** 2).sum((0, 2, 3)) / n
        stats[p + ".running_mean"] = ((1 - MOMENTUM) * rm + MOMENTUM * mean).detach()
        stats[p + ".running_var"] = ((1 - MOMENTUM) * rv + MOMENTUM * var * (1.0 if biased_running else n / max(n - 1, 1))).detach()
        if no_mean_term:
            mean = mean.detach()
        return (c - mean[None, :, None, None]) * (w / torch.sqrt(var + EPS))[None, :, None, None] + b[None, :, None, None]

    def conv(y, w, stride, pad, short=False):
        if short:                                    # the weight gradient stops before the last image
            live = torch.ones(N, 1, 1, 1, dtype=dt)
            live[-1] = 0
            part = F.conv2d(y.detach(), w, None, stride, pad)
            return F.conv2d(y, w.detach(), None, stride, pad) + live * (part - part.detach())
        return F.conv2d(y, w, None, stride, pad)

    def relu(z, name):
        pre[name] = z
        m = masks[name] if masks is not None else z.detach() > 0
        used[name] = m
        return z * m.to(dt)

    kw = dict(biased_running=mutant == "running_var_biased", no_mean_term=mutant == "bn_bwd_no_mean_term")
    wide = dict(skip=mutant == "stats_skip_rows_128", count_padded=mutant == "stats_count_padded")
    short = mutant == "wgrad_short_of_last_image"
    # stem: the frame is repeated to 3 channels, so the 3 input channels of the weights are summed
    z0 = bn(conv(x[:, None], sd["0.weight"].sum(1, keepdim=True), 2, 3, short), "1", **kw)
    zp = z0
    if mutant == "pool_drops_last":                  # the last row / column of an odd stem grid never reaches a window
        zp = z0.clone()
        if z0.shape[2] % 2:
            zp[:, :, -1] = -1.0
        if z0.shape[3] % 2:
            zp[:, :, :, -1] = -1.0
    zw = pool_windows(zp, 0.0)                                           # (gathered from: zero outside the image, never picked)
    yw = pool_windows(zp.detach().clamp(min=0), float("-inf"))           # post-ReLU, -inf outside the image
    am = argmax.long() if argmax is not None else yw.argmax(0)
    pooled = zw.gather(0, am[None])[0]
    if mutant == "pool_second_best":
        second = yw.scatter(0, am[None], float("-inf")).argmax(0)
        pooled = _mix(pooled, zw.gather(0, second[None])[0])
    pre["pool"] = pool_windows(zp, float("-inf")).max(0)[0]
    mp = masks["pool"] if masks is not None else pooled.detach() > 0
    used["pool"] = mp
    y = pooled * mp.to(dt)
    if mutant == "pool_hw_swapped":                  # the flat index of a pooled element decoded with Hp where Wp belongs
        Hp, Wp = y.shape[2:]
        S = max(Hp, Wp)
        Hc, Wc = z0.shape[2:]
        ext = F.max_pool2d(F.pad(z0.clamp(min=0), (1, 2 * S - Wc, 1, 2 * S - Hc)), 3, 2, 0)
        ext = ext * ((torch.arange(S) < Hp)[:, None] & (torch.arange(S) < Wp)[None, :]).to(dt)
        flat = torch.arange(Hp * Wp)
        y = ext[:, :, (flat // Hp).clamp(max=S - 1), flat % Hp].reshape(N, 64, Hp, Wp) * ((flat // Hp) < S).to(dt).reshape(Hp, Wp)
        used["pool"] = y.detach() > 0
    cin = 64
    for li, (c, stride) in enumerate(resnet18.STAGES):
        for bi in range(2):
            p = "%d.%d" % (4 + li, bi)
            s = stride if bi == 0 else 1
            k = wide if c >= 128 else {}
            yin = y
            if mutant == "s2_dgrad_misses_last" and s == 2:      # dx of the 3x3 stride-2 product without the last row / column
                live = torch.ones(1, 1, y.shape[2], y.shape[3], dtype=dt)
                if y.shape[2] % 2 == 0:
                    live[:, :, -1] = 0
                if y.shape[3] % 2 == 0:
                    live[:, :, :, -1] = 0
                yin = _mix(y, y * live)
            z1 = bn(conv(yin, sd[p + ".conv1.weight"], s, 1, short and li == 0), p + ".bn1", **kw, **k)
            if mutant == "a1_mask_from_output":
                pre[p + ".a1"] = z1
                used[p + ".a1"] = masks[p + ".a1"] if masks is not None else z1.detach() > 0
                box = [None]
                o = _MaskedBy.apply(z1, used[p + ".a1"].to(dt), box)
            else:
                o = relu(z1, p + ".a1")
            z2 = bn(conv(o, sd[p + ".conv2.weight"], 1, 1, short and li == 0), p + ".bn2", **kw, **k)
            idn = y
            if s != 1 or cin != c:
                cd = conv(y, sd[p + ".downsample.0.weight"], s, 0)
                idn = bn(cd, p + ".downsample.1", **kw, **k)
                if mutant == "identity_before_ds_bn":
                    idn = cd + 0.0 * idn
            y = relu(z2 + idn, p)
            if mutant == "a1_mask_from_output":
                box[0] = used[p]
            cin = c
    feat = y.mean((2, 3))
    return types.SimpleNamespace(feat=feat, stats=stats, pre=pre, z0=z0, masks=used, argmax=am)


def run(case, dtype, masks=None, argmax=None, frozen=(), accumulate=False, mutant=None, keep_pre=True):
    """forward + backward of sum(feat * G) in ``dtype`` -> namespace(feat, grads, stats, masks, argmax, pre, z0); grads maps
    the 60 parameter keys to gradients, None for what ``frozen`` names"""
    inp = inputs(case)
    sd = {k: v.to(dtype).clone() if v.is_floating_point() else v for k, v in inp.sd.items()}
    params = {k: sd[k].requires_grad_(k not in frozen) for k in param_keys()}
    if accumulate:
        for k, v in params.items():
            if k not in frozen:
                v.grad = prefill(k, v.shape).to(dtype)
    r = trunk_restated(sd, inp.x.to(dtype), inp.training, masks, argmax, mutant)
    (r.feat * inp.G.to(dtype)).sum().backward()
    return types.SimpleNamespace(
        feat=r.feat.detach(), grads={k: v.grad for k, v in params.items()}, stats=r.stats, masks=r.masks,
        argmax=r.argmax.to(torch.uint8), pre={k: v.detach() for k, v in r.pre.items()} if keep_pre else None,
        z0=r.z0.detach() if keep_pre else None)


@functools.lru_cache(maxsize=2)
def reference(case):
    """the float64 evaluation under its own decisions (the test modules walk case by case: two cases stay cached)"""
    return run(case, torch.float64)


def trunk_fp32(inp, frozen=(), accumulate=False, mutant=None, masks=None, argmax=None):
    """the float32 CPU stand-in: the restatement in float32 under its own decisions (pinned to ``oracle.resnet18`` by
    tests/test_trunk_cpu.py)"""
    r = run(inp.case, torch.float32, masks, argmax, frozen, accumulate, mutant, keep_pre=False)
    return dict(feat=r.feat, grads=r.grads, stats=r.stats, masks=r.masks, argmax=r.argmax)


# ------------------------------------------------------------------------------------------ the assertion
def units(case):
    c = CASES[case]
    h, w = (c["H"] - 1) // 2 + 1, (c["W"] - 1) // 2 + 1
    n = 0
    for s, ch in enumerate((64, 128, 256, 512)):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        n += c["N"] * h * w * ch * (5 if s == 0 else 4)
    return n


def cap(case):
    return 2 + units(case) // 1000000


def decisions(got, ref, case):
    """-> (differing ReLU units, differing pool positions, violations): violations name every decision of ``got`` that
    differs from float64's (the evaluation ``ref``) outside the rule"""
    t = tau(case)
    n_relu = n_pool = 0
    bad = []
    for k in NAMES:
        m, p = got["masks"][k].cpu(), ref.pre[k]
        assert m.dtype == torch.bool and tuple(m.shape) == tuple(p.shape), (k, m.dtype, tuple(m.shape), tuple(p.shape))
        diff = m != (p > 0)
        n = int(diff.sum())
        if n == 0:
            continue
        n_relu += n
        out = diff & (p.abs() > t[k])
        for idx in out.nonzero()[:4].tolist():
            bad.append("ReLU unit %s%s on the other side at |pre64| = %.3e > tau = %.1e" % (k, tuple(idx), abs(float(p[tuple(idx)])), t[k]))
        if int(out.sum()) > 4:
            bad.append("... and %d more in %s (of %d that differ)" % (int(out.sum()) - 4, k, n))
    am = got["argmax"].cpu().long()
    yw = pool_windows(ref.z0.clamp(min=0), float("-inf"))
    assert tuple(am.shape) == tuple(yw.shape[1:]), (tuple(am.shape), tuple(yw.shape[1:]))
    assert int(am.max()) <= 8, "pool arg-max %d is no window position" % int(am.max())
    diff = am != yw.argmax(0)
    n_pool = int(diff.sum())
    if n_pool:
        gap = yw.max(0)[0] - yw.gather(0, am[None])[0]
        out = diff & ~(gap <= t["pool"])
        for idx in out.nonzero()[:4].tolist():
            bad.append("pool window %s takes position %d, %.3e below float64's maximum > tau = %.1e" % (
                tuple(idx), int(am[tuple(idx)]), float(gap[tuple(idx)]), t["pool"]))
        if int(out.sum()) > 4:
            bad.append("... and %d more pool windows (of %d that differ)" % (int(out.sum()) - 4, n_pool))
    return n_relu, n_pool, bad


def check_trunk(impl, case, frozen=(), options_label="", accumulate=False, tag="gpu"):
    """``impl(inp, frozen)`` -> dict(feat (N,512), grads {60 keys: gradient of sum(feat * inp.G), None if frozen; with
    ``accumulate`` added to ``prefill``}, stats {40 keys: the running statistics after the forward}, masks {17 names: bool},
    argmax (N,64,h2,w2) uint8).  See the module docstring.  -> (differing ReLU decisions, differing pool positions)."""
    inp = inputs(case)
    got = impl(inp, tuple(frozen))
    ref = reference(case)
    t = "%s%s%s%s " % (case, " " + options_label if options_label else "", " [frozen: %d]" % len(frozen) if frozen else "",
                       " [accumulate]" if accumulate else "")
    n_relu, n_pool, bad = decisions(got, ref, case)
    if n_relu or n_pool:
        ref = run(case, torch.float64, masks={k: got["masks"][k].cpu() for k in NAMES}, argmax=got["argmax"].cpu())
        n_relu, n_pool, bad = decisions(got, ref, case)
    if tag is not None:
        H.log_line("head %-5s %-8s %sdecisions that differ from float64: %d ReLU + %d pool of %d units (cap %d)" % (
            tag, FAMILY, t, n_relu, n_pool, units(case), cap(case)))
    assert not bad, t + "\n".join(bad)
    assert n_relu + n_pool <= cap(case), "%s%d ReLU + %d pool decisions differ from float64: more than the cap %d" % (t, n_relu, n_pool, cap(case))
    H.report(FAMILY + ".f", t + "features", got["feat"], ref.feat, FEAT_BOUND * max(1.0, float(ref.feat.abs().max())), tag=tag)
    assert set(got["stats"]) == set(ref.stats), sorted(set(got["stats"]) ^ set(ref.stats))
    for k in sorted(ref.stats):
        H.report(FAMILY + ".s", t + k, got["stats"][k], ref.stats[k], 1e-5, 1e-5, tag=tag)
    grads = got["grads"]
    assert set(grads) == set(ref.grads), sorted(set(grads) ^ set(ref.grads))
    failed = []
    for k in param_keys():
        if k in frozen:
            assert grads[k] is None, t + k + " is frozen and has a gradient"
            continue
        assert grads[k] is not None, t + k + " has no gradient"
        g, r = grads[k].detach().cpu().double(), ref.grads[k]
        assert tuple(g.shape) == tuple(r.shape), (k, tuple(g.shape))
        if accumulate:                               # (the bound is the gradient's own, not the sum's)
            g = g - prefill(k, r.shape).double()
        try:
            H.report_grad(FAMILY + ".g", t + "d/d" + k, g, r, tag=tag)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "%s%d of %d gradients miss the bound\n%s" % (t, len(failed), len(param_keys()) - len(frozen), "\n".join(failed[:6]))
    if tag is not None:
        RUNS.append((tag, t.strip(), n_relu, n_pool, cap(case)))
    return n_relu, n_pool


def log_worst(tag):
    for (tg, family), (ratio, name) in sorted(H.WORST.items()):
        if tg == tag and family.startswith(FAMILY):
            H.log_line("head %-5s %-8s WORST ratio=%.4f  (%s)" % (tag, family, ratio, name))
    runs = [r for r in RUNS if r[0] == tag]
    H.log_line("head %-5s %-8s runs: %d; decisions that differed: %s" % (
        tag, FAMILY, len(runs), "; ".join("%s: %d+%d/%d" % r[1:] for r in runs if r[2] or r[3]) or "none"))


# ------------------------------------------------------------------------------------------ the form choices, restated
# csrc/trunk.hip: make_plan's geometry, cls_tile_cap, stem_kernel_ok, stem_wgrad_ok, conv64_ok, conv64_wgrad_ok, the class
# predicates, fwd_form / dgrad_form / wgrad_form, fused_chunks and stat_ctx for the fp32 data path (slab always present).
OPTIONS = dict(no_cls=0, no_s2_cls=0, no_conv64=0, no_streamk=0, no_fused_stats=0, no_stem_kernel=0, no_tall=0, no_buf=0,
               no_fixup1=0, cls_cap=0, max_cus=0, bwd_max_cus=0)
STEM_WH, WG_MAXW, WG_PART, SLAB_FLOATS, STAT_CHUNKS, MAXC = 17, 18, 9 * 64 * 64, 256 * 576 * 64, 512, 1024


def cdiv(a, b):
    return -(-a // b)


def geoms(N, H, W):
    """the 20 convolutions in the order of include/avvad.h, as make_plan lays them out"""
    h, w = [H, (H - 1) // 2 + 1], [W, (W - 1) // 2 + 1]
    for _ in range(4):
        h.append((h[-1] - 1) // 2 + 1)
        w.append((w[-1] - 1) // 2 + 1)
    g = [dict(name="0", N=N, H=h[0], W=w[0], C=1, Ho=h[1], Wo=w[1], Co=64, KS=7, stride=2, pad=3)]
    cin = 64
    for s, c in enumerate((64, 128, 256, 512)):
        for b in range(2):
            ds = b == 0 and s > 0
            hin, win = (h[s + 1], w[s + 1]) if ds else (h[s + 2], w[s + 2])
            ho, wo = h[s + 2], w[s + 2]
            p = "%d.%d" % (4 + s, b)
            g.append(dict(name=p + ".conv1", N=N, H=hin, W=win, C=cin, Ho=ho, Wo=wo, Co=c, KS=3, stride=2 if ds else 1, pad=1))
            g.append(dict(name=p + ".conv2", N=N, H=ho, W=wo, C=c, Ho=ho, Wo=wo, Co=c, KS=3, stride=1, pad=1))
            if ds:
                g.append(dict(name=p + ".downsample.0", N=N, H=hin, W=win, C=cin, Ho=ho, Wo=wo, Co=c, KS=1, stride=2, pad=0))
            cin = c
    return [types.SimpleNamespace(**d) for d in g]


def fits_buf(n):
    return 0 <= n < (1 << 29) - 64


def _cus(o):
    return o["max_cus"] if 0 < o["max_cus"] < 256 else 256


def cls_tile_cap(o):
    return o["cls_cap"] if o["cls_cap"] > 0 else 4 * _cus(o)


def stem_kernel_ok(g, o):
    ldw = (g.W + 6) | 1
    return (g.C, g.KS, g.stride, g.pad, g.Co) == (1, 7, 2, 3, 64) and (g.H + 6) * ldw * 4 <= 48 * 1024 and not o["no_stem_kernel"]


def stem_wgrad_ok(g, o):
    return stem_kernel_ok(g, o) and g.Wo % 2 == 0 and g.Wo <= 2 * STEM_WH and g.Ho * g.Wo * 64 * 4 < (1 << 31)


def cls_common(g, o):
    return (not o["no_cls"] and g.KS == 3 and g.pad == 1 and g.N >= 128 and g.C % 32 == 0 and g.Co % 32 == 0 and g.Ho >= 2 and
            g.Wo >= 2 and not o["no_buf"] and o["no_streamk"] == 0)


def conv_fwd_cls_ok(g, o):
    if not cls_common(g, o) or g.Co % 4 or g.Co < 128:
        return False
    return (g.Ho * g.Wo * cdiv(g.N, 128) * cdiv(g.Co, 128) <= cls_tile_cap(o) and fits_buf(g.N * g.H * g.W * g.C) and
            fits_buf(9 * g.C * g.Co))


def conv_dgrad_cls_ok(g, o):
    if not cls_common(g, o) or (g.stride != 1 and (g.stride != 2 or o["no_s2_cls"])) or g.C % 4 or g.C < 128:
        return False
    return (g.H * g.W * cdiv(g.N, 128) * cdiv(g.C, 128) <= cls_tile_cap(o) and fits_buf(g.N * g.Ho * g.Wo * g.Co) and
            fits_buf(9 * g.C * g.Co))


def conv_wgrad_tap_ok(g, o):
    if not cls_common(g, o) or g.C % 128 or g.Co % 4 or g.Co < 128:
        return False
    return (9 * (g.C // 128) * cdiv(g.Co, 128) <= cls_tile_cap(o) and fits_buf(g.N * g.H * g.W * g.C) and
            fits_buf(g.N * g.Ho * g.Wo * g.Co))


def conv64_ok(g, o):
    M = g.N * g.H * g.W
    return (not o["no_conv64"] and (g.C, g.Co, g.KS, g.stride, g.pad) == (64, 64, 3, 1, 1) and (g.Ho, g.Wo) == (g.H, g.W) and
            M > 0 and fits_buf(M * 64) and (M + 64) * g.H * g.W < (1 << 32))


def conv64_wgrad_ok(g, o):
    return conv64_ok(g, o) and g.W <= WG_MAXW and _cus(o) * WG_PART <= SLAB_FLOATS and g.N * g.H * g.W * 256 < (1 << 31)


def _engine(form, rows, cols, buf):
    return "%s %dx%d%s" % (form, rows, cols, " buf" if buf else "")


def fwd_form(g, o):
    """-> (form, partial-sum chunks its epilogue leaves)"""
    M = g.N * g.Ho * g.Wo
    cols = 64 if g.Co <= 64 else 128
    if conv64_ok(g, o):
        T = cdiv(g.N * g.H * g.W, 32)
        return "CONV64", min(max(T, 1), _cus(o))
    if conv_fwd_cls_ok(g, o):
        return "CLS", g.Ho * g.Wo * cdiv(g.N, 128)
    if g.C == 1:
        return ("STEM", g.N) if stem_kernel_ok(g, o) else (_engine("ENGINE", 128, 64, False), 0)
    rows = 256 if g.Co <= 64 and not o["no_tall"] else 128
    buf = fits_buf(g.N * g.H * g.W * g.C) and fits_buf(g.KS * g.KS * g.C * g.Co) and not o["no_buf"]
    return _engine("ENGINE", rows, cols, buf), cdiv(M, rows)


def dgrad_form(g, o):
    if conv64_ok(g, o):
        return "CONV64"
    if conv_dgrad_cls_ok(g, o):
        return "CLS"
    cols = 64 if g.C <= 64 else 128
    buf = fits_buf(g.N * g.Ho * g.Wo * g.Co) and fits_buf(g.KS * g.KS * g.C * g.Co) and not o["no_buf"]
    if g.stride == 2:
        return _engine("PARITY", 128, cols, buf)
    return _engine("ENGINE", 256 if cols == 64 and not o["no_tall"] else 128, cols, buf)


def wgrad_form(g, o):
    cols = 64 if g.Co <= 64 else 128
    if conv64_wgrad_ok(g, o):
        return "CONV64"
    if conv_wgrad_tap_ok(g, o):
        return "TAP"
    if g.C == 1:
        return "STEM" if stem_wgrad_ok(g, o) else _engine("ENGINE", 64, 64, False)
    buf = fits_buf(g.N * g.H * g.W * g.C) and fits_buf(g.N * g.Ho * g.Wo * g.Co) and not o["no_buf"]
    return _engine("ENGINE", 128, cols, buf)


def stat_ctx(M, C):
    """-> (chunks, rows per chunk) of the separate column-reduction pass"""
    RL = 256 // (C // 4)
    per = max(cdiv(M, STAT_CHUNKS), 16 * RL)
    per = cdiv(per, RL) * RL
    return cdiv(M, per), per


def fused_chunks(g, o, training):
    if not training or o["no_fused_stats"]:
        return 0
    n = fwd_form(g, o)[1]
    return n if n * g.Co <= STAT_CHUNKS * MAXC else 0


def forms(case, **options):
    """one row (fwd, dgrad, wgrad, chunks) per convolution, keyed by its name: the kernel forms csrc/trunk.hip picks for
    ``case`` under ``options``; the backward's forms under its own CU cap (bwd_max_cus); the stem has no data gradient;
    chunks: the forward's fused statistics chunks, or "col N" for the separate pass of N chunks, None in eval mode"""
    c = CASES[case]
    assert set(options) <= set(OPTIONS), options
    o = dict(OPTIONS, **options)
    ob = dict(o)
    if o["bwd_max_cus"] > 0 and (o["max_cus"] <= 0 or o["bwd_max_cus"] < o["max_cus"]):
        ob["max_cus"] = o["bwd_max_cus"]
    rows = {}
    for i, g in enumerate(geoms(c["N"], c["H"], c["W"])):
        n = fused_chunks(g, o, c["training"])
        chunks = None if not c["training"] else (n if n else "col %d" % stat_ctx(g.N * g.Ho * g.Wo, g.Co)[0])
        rows[g.name] = (fwd_form(g, o)[0], None if i == 0 else dgrad_form(g, ob), wgrad_form(g, ob), chunks)
    return rows


def stem_bwd_grid(case, **options):
    """workgroups of stem_pool_relu_bwd (= chunks of the stem's fused BatchNorm-backward sums)"""
    c = CASES[case]
    o = dict(OPTIONS, **options)
    n = c["N"] * ((c["H"] - 1) // 2 + 1) * ((c["W"] - 1) // 2 + 1) * 16
    grid = min(max(cdiv(n, 256), 1), 4096)
    return min(grid, 2048) if not o["no_fused_stats"] else grid


# option variants: (label, options, cases, base).  tests/test_trunk_cpu.py asserts that each changes a row of ``forms``
# against ``base`` (the default options, but for no_tall: 256-row tiles serve only the 64-channel convolutions that
# no_conv64 sends to the engine, so the variant is no_conv64 + no_tall against no_conv64).  no_fixup1 changes no form, so
# it is no variant.
VARIANTS = [
    ("no_cls", dict(no_cls=1), ("T1", "T8"), {}),
    ("no_s2_cls", dict(no_s2_cls=1), ("T1", "T8"), {}),
    ("no_conv64", dict(no_conv64=1), ("T1", "T8", "T7"), {}),
    ("no_streamk", dict(no_streamk=1), ("T1", "T8"), {}),
    ("no_fused_stats", dict(no_fused_stats=1), ("T1", "T8", "T7"), {}),
    ("no_stem_kernel", dict(no_stem_kernel=1), ("T1", "T8", "T7"), {}),
    ("no_tall", dict(no_conv64=1, no_tall=1), ("T1", "T8", "T7"), dict(no_conv64=1)),
    ("no_buf", dict(no_buf=1), ("T1", "T8", "T7"), {}),
    ("cls_cap40", dict(cls_cap=40), ("T1", "T8"), {}),
    ("max_cus200", dict(max_cus=200), ("T1", "T8"), {}),
    ("bwd_max_cus8", dict(bwd_max_cus=8), ("T1", "T8"), {}),
]
