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
130 x 35x43, cap 10.)

The bf16 data path (option "bf16" = 1) has its own reference at the end of this module: a replay that is pinned to the
implementation's stored bf16 VALUES, not only to its decisions (``trunk_restated(..., bf16=...)``, ``check_trunk_bf16``)."""
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


def trunk_restated(sd, x, training, masks=None, argmax=None, mutant=None, bf16=None):
    """``oracle.resnet18.trunk_forward`` on gray frames x (N,H,W) with every ReLU as ``z * mask`` and the pool as a gather.
    (``bf16``: the value-pinned replay of the bf16 data path, see ``trunk_restated_bf16`` at the end of this module.)
    sd: keys without prefix.  masks: name -> bool (N,C,H,W) for the 17 layers of NAMES; argmax: (N,64,Hp,Wp) window
    positions dh*3+dw.  Left out, they are this evaluation's own: z > 0 and the first maximum in scan order.
    -> namespace(feat, stats (updated running statistics, sd untouched), pre (the 17 pre-activations; "pool": the largest
    pre-activation of the window), z0 (the stem's pre-activation), masks, argmax)."""
    if bf16 is not None:
        assert masks is None
        return trunk_restated_bf16(sd, x, training, bf16, argmax, mutant)
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


# ========================================================================================== the bf16 data path (option "bf16" = 1)
# A VALUE-PINNED replay.  Under option "bf16" = 1 csrc/trunk.hip keeps the 17 post-ReLU activations as bf16, and bf16
# rounding is discontinuous: a free-running reference is a bf16 step away after one layer and 5 .. 9 % away in the deep
# gradients.  So the float64 replay CONTINUES WITH THE IMPLEMENTATION'S STORED VALUES: at storage point k it computes its own
# pre-store value v_k from the implementation's stored inputs of that layer, the stored value s_k is held to v_k by the
# forward rule, and the next layer takes s_k (the gradient path goes through v_k, ``_mix``).  Every layer is compared given
# exact inputs, nothing compounds, a failure names layer and index, and the backward is the exact backward of the network
# the implementation ran.
#
# Where the implementation rounds (read from csrc/trunk.hip, bn_kernels.h, bgemm.h, conv64.h, igemm.h):
# * weights: convolutions 1 .. 19 multiply rne_bf16(w) (pack_all's bf16 packs, forward and data gradient alike); their
#   gradient goes straight through to the fp32 master weight;
# * the stem (convolution 0) runs the fp32 entry points whatever the option: its LDS kernels (stem_fwd_mfma, stem_wgrad_mfma)
#   are fp32, its engine fall-backs go through igemm::launch, which under the option rounds BOTH operands to bf16 while
#   staging.  Per form (``stem_rounding``, asserted by the CPU test): forward STEM -> exact, ENGINE -> rne(x) * rne(sum_c w);
#   weight gradient STEM -> exact, ENGINE -> rne(x) * rne(d c0); the stem has no data gradient.  T5 runs the forward on the
#   stem kernel and the weight gradient on the engine;
# * forward stores: the 17 activations are rne_bf16(relu(fp32 value)) (stem_bn_relu_pool<true>, bn_act<true, .>); raw
#   convolution outputs, batch statistics, the downsample branch's identity (bn_act reads the raw fp32 output of the 1x1
#   convolution) and the features are fp32; a block input that serves as identity is read back as the stored bf16 value;
#   the byte mask (and the pool / a1 masks the backward rebuilds) is the sign of the fp32 value before the store, which is the
#   sign of the stored value (rne keeps a positive fp32 positive);
# * backward stores: bn_bwd_apply<true> stores d(raw convolution output) as bf16 for every convolution behind the stem, and
#   that one value feeds the data gradient and the weight gradient (``_RoundGrad`` on each raw output: identity forward,
#   rne in the backward); gout, the data-gradient outputs and the whole stem backward are fp32.
#
# THE FORWARD RULE, per element: rne(relu(v - d_k)) <= s <= rne(relu(v + d_k)): one or two adjacent bf16 values (all values
# up to rne(2 d_k) where |v| < d_k: a ReLU unit within rounding of zero).  Round-toward-zero, a double rounding and a missing
# ReLU fall outside.  d_k = D16[case][k] is 10 x the largest |v32 - v64| of the float32 stand-in at that layer under the same
# pinning (tests/test_trunk_bf16_cpu.py asserts 8 .. 16 x, the margin and reason of TAU).  D16's first entry is the stem's
# pre-activation z0 as it runs under the option: the pool-position rule's tau.
# VALUES, element-wise, no aggregate: features against the mean of the implementation's last stored activation,
# 2e-5 max(1, max|ref|); the 40 running statistics 1e-5 + 1e-5 |ref|; the 60 gradients B16 max(1, max|ref|) with
# B16 = max(1e-4, 10 x E32), E32 the float32 stand-in's worst such distance over all cases and gradients: a cotangent that
# fp32 noise puts on the other bf16 neighbour moves by 2^-8 relative.
FAMILY16 = "trunk16"
D_NAMES = ["z0"] + NAMES
TWO_VALUE_CAP = 0.05          # most elements of a layer whose admissible set holds two values (CPU test, on float64's own values)
RUNS16 = []                   # (tag, label, largest two-value share of a layer, far-neighbour elements, elements) per passing run
MUTANTS16 = ("store_truncates", "bn2_rounded_before_add", "ds_identity_rounded", "input_fp32_pitch", "mask_bits_reversed",
             "mask_shifted_quad", "stats_skip_rows_128", "dgrad_pack_via_fp16", "dgrad_weights_unrounded", "stem_rounds_operands")

# 10 x the measured float32 spread under the pinning, in the order of D_NAMES (tests/test_trunk_bf16_cpu.py)
D16 = {
    "T1": (3.5e-05, 3.5e-05, 2.7e-05, 1.5e-05, 2.1e-05, 2.0e-05, 2.2e-05, 3.4e-05, 1.9e-05, 1.5e-05, 2.0e-05, 2.1e-05, 1.8e-05, 2.0e-05, 1.9e-05, 2.8e-05, 2.5e-05, 2.3e-05),
    "T1e": (3.4e-05, 3.4e-05, 3.3e-05, 3.0e-05, 7.5e-05, 5.2e-05, 1.3e-04, 1.2e-04, 1.6e-04, 1.9e-04, 2.4e-04, 2.7e-04, 2.9e-04, 3.8e-04, 3.6e-04, 4.4e-04, 4.0e-04, 3.3e-04),
    "T2": (2.9e-05, 2.9e-05, 2.8e-05, 2.1e-05, 2.1e-05, 2.1e-05, 2.2e-05, 2.5e-05, 2.7e-05, 1.6e-05, 2.0e-05, 2.2e-05, 1.8e-05, 1.9e-05, 2.3e-05, 2.5e-05, 1.8e-05, 1.9e-05),
    "T3": (3.0e-05, 2.8e-05, 2.0e-05, 1.9e-05, 2.7e-05, 2.4e-05, 1.7e-05, 2.6e-05, 2.6e-05, 1.8e-05, 1.9e-05, 2.0e-05, 1.7e-05, 1.8e-05, 2.0e-05, 2.3e-05, 2.1e-05, 2.3e-05),
    "T4": (2.6e-05, 2.5e-05, 2.5e-05, 1.6e-05, 2.2e-05, 1.8e-05, 3.4e-05, 2.9e-05, 1.7e-05, 1.9e-05, 2.1e-05, 2.2e-05, 1.6e-05, 1.6e-05, 1.2e-05, 1.9e-05, 1.7e-05, 1.3e-05),
    "T5": (2.9e-05, 2.9e-05, 2.1e-05, 1.7e-05, 2.4e-05, 2.2e-05, 3.0e-05, 3.0e-05, 1.8e-05, 1.9e-05, 2.3e-05, 2.6e-05, 2.3e-05, 2.3e-05, 1.9e-05, 2.6e-05, 2.1e-05, 2.1e-05),
    "T6": (3.2e-05, 2.6e-05, 2.2e-05, 2.3e-05, 2.9e-05, 3.1e-05, 2.6e-05, 2.7e-05, 2.5e-05, 2.4e-05, 2.7e-05, 3.7e-05, 2.6e-05, 2.5e-05, 2.7e-05, 3.1e-05, 2.4e-05, 2.3e-05),
    "T7": (1.8e-05, 1.8e-05, 1.2e-05, 1.1e-05, 1.2e-05, 1.0e-05, 9.9e-06, 1.1e-05, 1.1e-05, 8.4e-06, 1.1e-05, 1.4e-05, 1.0e-05, 1.0e-05, 9.8e-06, 1.5e-05, 1.1e-05, 1.2e-05),
    "T7e": (2.3e-05, 2.3e-05, 2.2e-05, 2.4e-05, 5.6e-05, 3.6e-05, 1.3e-04, 1.1e-04, 1.2e-04, 1.4e-04, 1.8e-04, 2.0e-04, 2.0e-04, 1.8e-04, 2.1e-04, 4.0e-04, 3.0e-04, 2.1e-04),
    "T8": (3.4e-05, 3.1e-05, 2.3e-05, 2.2e-05, 2.1e-05, 2.5e-05, 1.8e-05, 2.8e-05, 1.8e-05, 1.9e-05, 2.0e-05, 2.8e-05, 2.6e-05, 2.2e-05, 2.3e-05, 2.9e-05, 2.6e-05, 1.9e-05),
}
E32 = 1.1e-2                 # measured 1.13e-2 (T5, d/d 4.0.bn1.weight); 0.9 .. 1.1e-2 in training mode, 3.5e-3 in eval mode
B16 = max(1e-4, 10 * E32)


def d16(case):
    return dict(zip(D_NAMES, D16[case]))


_DROP = 45                    # float64 keeps 52 mantissa bits, bf16 7


def rne_bf16(t):
    """round to nearest even to bf16 precision, in t's dtype (float64: ONE rounding, on the bits; values below bf16's normal
    range, 1.2e-38, keep more bits than bf16 has)"""
    if t.dtype != torch.float64:
        return t.bfloat16().to(t.dtype)
    b = t.contiguous().view(torch.int64)
    return ((b + ((b >> _DROP) & 1) + ((1 << (_DROP - 1)) - 1)) & ~((1 << _DROP) - 1)).view(torch.float64)


def trunc_bf16(t):
    if t.dtype != torch.float64:
        return (t.float().contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(t.dtype)
    return (t.contiguous().view(torch.int64) & ~((1 << _DROP) - 1)).view(torch.float64)


class _RoundGrad(torch.autograd.Function):
    """identity forward; the cotangent is stored as bf16 (bn_bwd_apply<true>)"""

    @staticmethod
    def forward(ctx, c):
        return c.view_as(c)

    @staticmethod
    def backward(ctx, g):
        return rne_bf16(g)


def _quads(m, f):
    """f on the (quads, 4) view of an (N,C,H,W) mask in the kernels' NHWC order"""
    n, c, h, w = m.shape
    return f(m.permute(0, 2, 3, 1).reshape(-1, 4)).reshape(n, h, w, c).permute(0, 3, 1, 2)


def trunk_restated_bf16(sd, x, training, cfg, argmax=None, mutant=None):
    """the bf16 data path restated (see above).  cfg: namespace(acts: name -> the stored values (N,C,H,W) of the 17 layers to
    continue with, or None: this evaluation's own, rne(relu(v)); stem: subset of {"fwd", "wgrad"}, the stem products that run
    on the engine).  -> namespace(feat, stats, v (the 17 pre-ReLU pre-store values), z0, acts, masks, argmax)"""
    assert mutant is None or mutant in MUTANTS16, mutant
    dt = x.dtype
    pin = cfg.acts
    stats, v, acts, used = {}, {}, {}, {}
    rnd = trunc_bf16 if mutant == "store_truncates" else rne_bf16

    def bn(c, p, skip=False):
        w, b, rm, rv = sd[p + ".weight"], sd[p + ".bias"], sd[p + ".running_mean"], sd[p + ".running_var"]
        if not training:
            stats[p + ".running_mean"], stats[p + ".running_var"] = rm.detach().clone(), rv.detach().clone()
            return (c - rm[None, :, None, None]) * (w / torch.sqrt(rv + EPS))[None, :, None, None] + b[None, :, None, None]
        src = c[:128] if skip else c
        n = src.numel() // src.shape[1]
        mean = src.sum((0, 2, 3)) / n
        var = ((src - mean[None, :, None, None]) ** 2).sum((0, 2, 3)) / n
        stats[p + ".running_mean"] = ((1 - MOMENTUM) * rm + MOMENTUM * mean).detach()
        stats[p + ".running_var"] = ((1 - MOMENTUM) * rv + MOMENTUM * var * (n / max(n - 1, 1))).detach()
        return (c - mean[None, :, None, None]) * (w / torch.sqrt(var + EPS))[None, :, None, None] + b[None, :, None, None]

    def wq(w, via_fp16=False):
        w0 = w.detach()
        if via_fp16:
            w0 = w0.half().to(dt)
        return _mix(rne_bf16(w0), w)

    def conv(y, w, stride, pad):
        if mutant in ("dgrad_weights_unrounded", "dgrad_pack_via_fp16"):      # the data gradient multiplies other weights
            wd = w.detach() if mutant == "dgrad_weights_unrounded" else wq(w, True).detach()
            dpath = F.conv2d(y, wd, None, stride, pad)
            c = F.conv2d(y.detach(), wq(w), None, stride, pad) + (dpath - dpath.detach())
        else:
            c = F.conv2d(y, wq(w), None, stride, pad)
        return _RoundGrad.apply(c)

    def store(vk, name, bwd_mask=None):
        v[name] = vk
        s = pin[name].to(dt) if pin is not None else rnd(vk.detach().clamp(min=0))
        m = s > 0
        acts[name], used[name] = s, m
        return _mix(s, vk * (m if bwd_mask is None else bwd_mask(m)).to(dt))

    bwd = None
    if mutant == "mask_bits_reversed":
        bwd = lambda m: _quads(m, lambda q: q.flip(1))
    if mutant == "mask_shifted_quad":
        bwd = lambda m: _quads(m, lambda q: q.roll(1, 0))
    # stem: value and gradient path apart, as the forward and the weight gradient may run on different forms
    w0 = sd["0.weight"].sum(1, keepdim=True)
    x1 = x[:, None]
    if "fwd" in cfg.stem or mutant == "stem_rounds_operands":
        c0 = F.conv2d(rne_bf16(x1), rne_bf16(w0.detach()), None, 2, 3)
    else:
        c0 = F.conv2d(x1, w0.detach(), None, 2, 3)
    gp = _RoundGrad.apply(F.conv2d(rne_bf16(x1), w0, None, 2, 3)) if "wgrad" in cfg.stem else F.conv2d(x1, w0, None, 2, 3)
    z0 = bn(_mix(c0, gp), "1")
    zw = pool_windows(z0, 0.0)
    yw = pool_windows(z0.detach().clamp(min=0), float("-inf"))
    am = argmax.long() if argmax is not None else yw.argmax(0)
    y = store(zw.gather(0, am[None])[0], "pool")
    cin = 64
    for li, (c, stride) in enumerate(resnet18.STAGES):
        for bi in range(2):
            p = "%d.%d" % (4 + li, bi)
            s = stride if bi == 0 else 1
            k = dict(skip=mutant == "stats_skip_rows_128") if c >= 128 else {}
            o = store(bn(conv(y, sd[p + ".conv1.weight"], s, 1), p + ".bn1", **k), p + ".a1")
            z2 = bn(conv(o, sd[p + ".conv2.weight"], 1, 1), p + ".bn2", **k)
            if mutant == "bn2_rounded_before_add":
                z2 = _mix(rne_bf16(z2.detach()), z2)
            if s != 1 or cin != c:
                idn = bn(conv(y, sd[p + ".downsample.0.weight"], s, 0), p + ".downsample.1", **k)
                if mutant == "ds_identity_rounded":
                    idn = _mix(rne_bf16(idn.detach()), idn)
            else:
                idn = y
                if mutant == "input_fp32_pitch" and p == "5.1":      # the second half of every row comes from the next row
                    n_, c_, h_, w_ = y.shape
                    t = y.detach().permute(0, 2, 3, 1).reshape(-1, c_)
                    t = torch.cat([t[:, :c_ // 2], t.roll(-1, 0)[:, :c_ // 2]], 1)
                    idn = _mix(t.reshape(n_, h_, w_, c_).permute(0, 3, 1, 2), y)
            y = store(z2 + idn, p, bwd)
            cin = c
    return types.SimpleNamespace(feat=y.mean((2, 3)), stats=stats, v=v, z0=z0, acts=acts, masks=used, argmax=am)


def run16(case, dtype, acts=None, argmax=None, frozen=(), accumulate=False, mutant=None, stem=None):
    """forward + backward of sum(feat * G) of the bf16 restatement in ``dtype`` (``acts``: pinned to these stored values)"""
    inp = inputs(case)
    sd = {k: v.to(dtype).clone() if v.is_floating_point() else v for k, v in inp.sd.items()}
    params = {k: sd[k].requires_grad_(k not in frozen) for k in param_keys()}
    if accumulate:
        for k, v in params.items():
            if k not in frozen:
                v.grad = prefill(k, v.shape).to(dtype)
    cfg = types.SimpleNamespace(acts=acts, stem=stem_rounding(case) if stem is None else stem)
    r = trunk_restated(sd, inp.x.to(dtype), inp.training, argmax=argmax, mutant=mutant, bf16=cfg)
    (r.feat * inp.G.to(dtype)).sum().backward()
    return types.SimpleNamespace(
        feat=r.feat.detach(), grads={k: v.grad for k, v in params.items()}, stats=r.stats, acts=r.acts,
        argmax=r.argmax.to(torch.uint8), v={k: t.detach() for k, t in r.v.items()}, z0=r.z0.detach())


def trunk_bf16_standin(inp, frozen=(), accumulate=False, mutant=None, stem=None):
    """the float32 CPU stand-in of the bf16 data path: the restatement in float32 with .bfloat16().float() at the storage
    points, under its own stored values and decisions"""
    r = run16(inp.case, torch.float32, None, None, frozen, accumulate, mutant, stem)
    return dict(feat=r.feat, grads=r.grads, stats=r.stats, acts=r.acts, argmax=r.argmax, v=r.v, z0=r.z0)


def replay(case, got, stem=None):
    """the float64 replay pinned to the stored values and pool positions of ``got``"""
    return run16(case, torch.float64, {k: got["acts"][k].detach().cpu().double() for k in NAMES}, got["argmax"].cpu(), stem=stem)


def admissible(vk, d):
    """-> (lo, hi) of the forward rule"""
    return rne_bf16((vk - d).clamp(min=0)), rne_bf16((vk + d).clamp(min=0))


def two_value_shares(v, case):
    """per layer: the share of elements whose admissible set holds more than one value"""
    d = d16(case)
    out = []
    for k in NAMES:
        lo, hi = admissible(v[k], d[k])
        out.append(float((lo != hi).double().mean()))
    return out


def check_trunk_bf16(impl, case, frozen=(), options_label="", accumulate=False, tag="gpu", options=None):
    """``impl(inp, frozen)`` -> dict(feat, grads, stats as for ``check_trunk``; acts {17 names: the stored activations as exact
    float32 copies (N,C,H,W)}, argmax).  Every failing comparison is collected and raised as ONE AssertionError whose lines
    start with the check that failed ("stored", "pool", "rule", "features", "running statistics", "gradient").
    -> (elements with a two-value admissible set, elements on the far neighbour)"""
    inp = inputs(case)
    got = impl(inp, tuple(frozen))
    t = "%s%s%s%s " % (case, " " + options_label if options_label else "", " [frozen: %d]" % len(frozen) if frozen else "",
                       " [accumulate]" if accumulate else "")
    d = d16(case)
    for k in NAMES:                                  # what the accessor hands out: exact float32 copies of bf16 values
        a = got["acts"][k]
        assert a.dtype == torch.float32, "%sstored %s is %s" % (t, k, a.dtype)
        a = a.cpu()
        assert torch.equal(a.bfloat16().float(), a), "%sstored %s holds values that are no bf16 values" % (t, k)
        assert bool((a >= 0).all()), "%sstored %s holds negative values" % (t, k)
    ref = replay(case, got, stem_rounding(case, **(options or {})))
    fails = []
    am = got["argmax"].cpu().long()
    yw = pool_windows(ref.z0.clamp(min=0), float("-inf"))
    assert tuple(am.shape) == tuple(yw.shape[1:]), (tuple(am.shape), tuple(yw.shape[1:]))
    assert int(am.max()) <= 8, "pool arg-max %d is no window position" % int(am.max())
    diff = am != yw.argmax(0)
    n_pool = int(diff.sum())
    if n_pool:
        gap = yw.max(0)[0] - yw.gather(0, am[None])[0]
        out = diff & ~(gap <= d["z0"])
        for idx in out.nonzero()[:4].tolist():
            fails.append("pool: window %s takes position %d, %.3e below float64's maximum > tau = %.1e" % (
                tuple(idx), int(am[tuple(idx)]), float(gap[tuple(idx)]), d["z0"]))
    n_two = n_far = n_el = 0
    worst_share = 0.0
    for k in NAMES:
        vk, s = ref.v[k], got["acts"][k].cpu().double()
        assert tuple(s.shape) == tuple(vk.shape), (k, tuple(s.shape), tuple(vk.shape))
        lo, hi = admissible(vk, d[k])
        two, far = int((lo != hi).sum()), int((s != rne_bf16(vk.clamp(min=0))).sum())
        n_two, n_far, n_el = n_two + two, n_far + far, n_el + s.numel()
        worst_share = max(worst_share, two / s.numel())
        bad = (s < lo) | (s > hi)
        if tag is not None:
            H.log_line("head %-5s %-8s %s%-7s two-value %.4f  far neighbour %d of %d  outside the rule %d" % (
                tag, FAMILY16 + ".r", t, k, two / s.numel(), far, s.numel(), int(bad.sum())))
        for idx in bad.nonzero()[:3].tolist():
            i = tuple(idx)
            fails.append("rule: %s%s stored %.9g outside [%.9g, %.9g]: v64 = %.9g, d = %.1e" % (
                k, i, float(s[i]), float(lo[i]), float(hi[i]), float(vk[i]), d[k]))
        if int(bad.sum()) > 3:
            fails.append("rule: ... and %d more in %s" % (int(bad.sum()) - 3, k))

    def rep(what, *a, **kw):
        try:
            H.report(*a, tag=tag, **kw)
        except AssertionError as e:
            fails.append("%s: %s" % (what, e))
    rep("features", FAMILY16 + ".f", t + "features", got["feat"], ref.feat, FEAT_BOUND * max(1.0, float(ref.feat.abs().max())))
    assert set(got["stats"]) == set(ref.stats), sorted(set(got["stats"]) ^ set(ref.stats))
    for k in sorted(ref.stats):
        rep("running statistics", FAMILY16 + ".s", t + k, got["stats"][k], ref.stats[k], 1e-5, rtol=1e-5)
    grads = got["grads"]
    assert set(grads) == set(ref.grads), sorted(set(grads) ^ set(ref.grads))
    for k in param_keys():
        if k in frozen:
            assert grads[k] is None, t + k + " is frozen and has a gradient"
            continue
        assert grads[k] is not None, t + k + " has no gradient"
        g, r = grads[k].detach().cpu().double(), ref.grads[k]
        assert tuple(g.shape) == tuple(r.shape), (k, tuple(g.shape))
        if accumulate:
            g = g - prefill(k, r.shape).double()
        rep("gradient", FAMILY16 + ".g", t + "d/d" + k, g, r, B16 * max(1.0, float(r.abs().max())))
    if tag is not None:
        H.log_line("head %-5s %-8s %stwo-value elements %d, far neighbour %d, of %d; largest two-value share of a layer %.4f; "
                   "pool positions that differ %d" % (tag, FAMILY16, t, n_two, n_far, n_el, worst_share, n_pool))
    kinds = []                                       # at most 4 lines per check, so that no check's verdict is cut off
    for f in fails:
        if f.split(":")[0] not in kinds:
            kinds.append(f.split(":")[0])
    shown = [f for kd in kinds for f in [x for x in fails if x.split(":")[0] == kd][:4]]
    assert not fails, "%s%d comparisons fail\n%s" % (t, len(fails), "\n".join(shown))
    if tag is not None:
        RUNS16.append((tag, t.strip(), worst_share, n_far, n_el))
    return n_two, n_far


def log_worst16(tag):
    for (tg, family), (ratio, name) in sorted(H.WORST.items()):
        if tg == tag and family.startswith(FAMILY16):
            H.log_line("head %-5s %-8s WORST ratio=%.4f  (%s)" % (tag, family, ratio, name))
    runs = [r for r in RUNS16 if r[0] == tag]
    H.log_line("head %-5s %-8s runs: %d; largest two-value share / far-neighbour elements: %s" % (
        tag, FAMILY16, len(runs), "; ".join("%s: %.4f / %d of %d" % r[1:] for r in runs) or "none"))


# ------------------------------------------------------------------------------------------ the bf16 form choices, restated
# csrc/trunk.hip: bf16_conv_ok, cls16_common, conv_fwd16_cls_ok, conv_dgrad16_cls_ok, conv_wgrad16_tap_ok, conv64_ok(g, true)
# and the b16 rows of fwd_form / dgrad_form / wgrad_form.  The stem keeps its fp32 row.
def bf16_conv_ok(g):
    return (g.C % 64 == 0 and g.Co % 64 == 0 and g.KS * g.KS <= 32 and fits_buf(g.N * g.H * g.W * g.C // 2) and
            fits_buf(g.N * g.Ho * g.Wo * g.Co // 2) and fits_buf(g.KS * g.KS * g.C * g.Co // 2))


def cls16_common(g, o):
    return (not o["no_cls"] and g.KS == 3 and g.pad == 1 and g.N >= 128 and g.Ho >= 2 and g.Wo >= 2 and g.Ho * g.Wo <= 9 and
            o["no_streamk"] == 0)


def conv_fwd16_cls_ok(g, o):
    return cls16_common(g, o) and g.Co >= 128 and g.Ho * g.Wo * cdiv(g.N, 128) * cdiv(g.Co, 128) <= cls_tile_cap(o)


def conv_dgrad16_cls_ok(g, o):
    form = cls16_common(g, o) if g.stride == 1 else (g.stride == 2 and g.KS == 3 and g.pad == 1 and not o["no_cls"] and
                                                     not o["no_s2_cls"] and o["no_streamk"] == 0 and g.N >= 128)
    return bool(form) and g.C >= 128 and g.H * g.W * cdiv(g.N, 128) * cdiv(g.C, 128) <= cls_tile_cap(o)


def conv_wgrad16_tap_ok(g, o):
    return cls16_common(g, o) and g.C % 128 == 0 and g.Co >= 128 and 9 * (g.C // 128) * cdiv(g.Co, 128) <= cls_tile_cap(o)


def fwd_form16(g, o):
    cols = 64 if g.Co <= 64 else 128
    if conv64_ok(g, o):                              # (conv64_ok(g, true): whatever option bf16 says)
        return "CONV64", min(max(cdiv(g.N * g.H * g.W, 32), 1), _cus(o))
    if conv_fwd16_cls_ok(g, o):
        return "CLS", g.Ho * g.Wo * cdiv(g.N, 128)
    return _engine("ENGINE", 128, cols, True), cdiv(g.N * g.Ho * g.Wo, 128)


def dgrad_form16(g, o):
    if conv64_ok(g, o):
        return "CONV64"
    if conv_dgrad16_cls_ok(g, o):
        return "CLS"
    return _engine("PARITY" if g.stride == 2 else "ENGINE", 128, 64 if g.C <= 64 else 128, True)


def wgrad_form16(g, o):
    return "TAP" if conv_wgrad16_tap_ok(g, o) else _engine("ENGINE", 128, 64 if g.Co <= 64 else 128, True)


def forms16(case, **options):
    """``forms`` for the bf16 data path: the stem's row is the fp32 one (its launchers are the fp32 entry points)"""
    c = CASES[case]
    assert set(options) <= set(OPTIONS), options
    o = dict(OPTIONS, **options)
    ob = dict(o)
    if o["bwd_max_cus"] > 0 and (o["max_cus"] <= 0 or o["bwd_max_cus"] < o["max_cus"]):
        ob["max_cus"] = o["bwd_max_cus"]
    rows = {}
    for i, g in enumerate(geoms(c["N"], c["H"], c["W"])):
        if i == 0:
            rows[g.name] = forms(case, **options)[g.name]
            continue
        assert bf16_conv_ok(g), g.name
        n = 0
        if c["training"] and not o["no_fused_stats"]:
            n = fwd_form16(g, o)[1]
            n = n if n * g.Co <= STAT_CHUNKS * MAXC else 0
        chunks = None if not c["training"] else (n if n else "col %d" % stat_ctx(g.N * g.Ho * g.Wo, g.Co)[0])
        rows[g.name] = (fwd_form16(g, o)[0], dgrad_form16(g, ob), wgrad_form16(g, ob), chunks)
    return rows


def stem_rounding(case, **options):
    """which of the stem's products round their operands to bf16 under the option: those on the engine"""
    f = forms(case, **options)["0"]
    return frozenset((["fwd"] if f[0] != "STEM" else []) + (["wgrad"] if f[2] != "STEM" else []))


# option variants of the GPU test: (label, options, cases); the CPU test asserts that each changes a bf16 row of every case
VARIANTS16 = [
    ("no_cls", dict(no_cls=1), ("T1", "T8")),
    ("no_s2_cls", dict(no_s2_cls=1), ("T1", "T8")),
    ("no_conv64", dict(no_conv64=1), ("T1", "T7")),
    ("no_streamk", dict(no_streamk=1), ("T1",)),
    ("no_fused_stats", dict(no_fused_stats=1), ("T1", "T7")),
    ("bwd_max_cus8", dict(bwd_max_cus=8), ("T1", "T8")),
]
