"""The oracle of the fusion-head tests: float64 references of everything that runs behind the encoders -- the MCB fusion
(count sketch, circular convolution, signed square root, whole-tensor L2 norm, BatchNorm1d), the packed LSTM stack and the two
BCE losses -- the case lists, and one assertion function per family (``check_fusion``, ``check_pooling``, ``check_lstm``,
``check_masked_bce``, ``check_bce_2classes``).  An assertion function takes the implementation under test as a callable:
tests/test_head_gpu.py passes the HIP path, tests/test_head_cpu.py passes the float32 CPU oracle (the bounds must be within
reach of a correct float32 evaluation) and seeded mutants of it (every assertion must be able to fail).

The references are plain torch, dtype-generic, and are called with float64 tensors; ``oracle/head.py`` and ``oracle/fusion.py``
are used where they already state the operation.

Two properties of the fusion decide what its reference is:

* The signed square root has derivative 0.5 / sqrt(|y| + eps) with eps = 1e-8, so the rare pooled values |y| <~ 1e-5 turn a
  last-bit difference of y into a visible difference of the input gradients: at 128 rows a correct float32 evaluation is 2e-2
  (relative L2) from float64 in d/d audio.  The reference is therefore PINNED to the implementation's own pooled vector
  (``fusion_pinned``): the float64 post-processing and its backward are evaluated at ``y_impl``, and only then is the
  cotangent dY carried through the float64 pooling.  ``y_impl`` itself is compared with the float64 pooling.
* The FFT form (``oracle.fusion.mcb``) returns ~1e-17 where the pooled value is exactly 0, and sign(1e-17) sqrt(1e-8) = 1e-4
  is not 0.  The direct sum (``mcb_direct``) gives exact zeros like the kernel and is the reference wherever D <= 260; the FFT
  form serves the dense D >= 1000 cases and is pinned to the direct sum by tests/test_head_cpu.py.

Bounds (the project's): outputs 1e-4 absolute; pooled y and running statistics 1e-4 + 1e-5 |ref|; gradients element-wise
1e-4 max(1, max|ref|) with NO relative-L2 alternative (no ReLU in the head: nothing can flip); loss values
1e-6 + 1e-5 |ref|.  Every comparison goes through ``report``, which prints and appends error, bound and their ratio to
the parity log of tests/test_gpu_parity.py."""
import functools
import os
import types

import numpy as np
import torch

from oracle import fusion, head
from test_gpu_parity import OUT

LOG = os.path.join(OUT, "parity.log")              # the parity log ``test_gpu_parity._report`` appends to
EPS = 1e-8
MOMENTUM = 0.1
UPSTREAM = 3.0                # factor on the loss before backward(): the gradients pass scale_by_device_scalar
WORST = {}                    # (tag, family) -> (worst ratio error / bound, name of the comparison)


# ------------------------------------------------------------------------------------------ reporting
def report(family, name, got, ref, atol, rtol=0.0, tag="gpu"):
    """max over the elements of |got - ref| / (atol + rtol |ref|) must not exceed 1.  ``tag`` names the implementation in the
    log; tag None (the mutants) keeps the comparison out of the log and of ``WORST``."""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    ref = ref.detach().cpu().double().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(ref).all(), name + ": non-finite reference"
    err = np.abs(got - ref)
    bound = atol + rtol * np.abs(ref)
    ratio = float((err / bound).max()) if err.size else 0.0
    msg = "head %-5s %-8s %-44s max|d|=%.3e  max|ref|=%.3e  bound=%.1e+%.1e*|ref|  ratio=%.4f" % (
        tag or "", family, name, err.max() if err.size else 0.0, np.abs(ref).max() if ref.size else 0.0, atol, rtol, ratio)
    if tag is not None:
        print(msg)
        if not (ratio <= WORST.get((tag, family), (-1.0, ""))[0]):
            WORST[(tag, family)] = (ratio, name)
        try:
            os.makedirs(os.path.dirname(LOG), exist_ok=True)
            with open(LOG, "a") as f:
                f.write(msg + "\n")
        except OSError:
            pass
    assert np.isfinite(got).all(), name + ": non-finite values"
    assert ratio <= 1.0, msg
    return ratio


def report_grad(family, name, got, ref, tag="gpu"):
    """element-wise 1e-4 max(1, max|ref|): the suite's gradient bound without its relative-L2 alternative"""
    ref = ref.detach().cpu().double()
    return report(family, name, got, ref, 1e-4 * max(1.0, float(ref.abs().max()) if ref.numel() else 0.0), tag=tag)


def log_line(msg):
    print(msg)
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(msg + "\n")
    except OSError:
        pass


def log_worst(tag):
    """one line per family: the worst error / bound this process has seen for ``tag``"""
    for (tg, family), (ratio, name) in sorted(WORST.items()):
        if tg == tag:
            log_line("head %-5s %-8s WORST ratio=%.4f  (%s)" % (tag, family, ratio, name))


def _rand(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def _signs(rng, n):
    return torch.from_numpy((2 * rng.integers(0, 2, n) - 1).astype(np.float32))


# ------------------------------------------------------------------------------------------ pooling references
def mcb_direct(a, v, h1, s1, h2, s2, D, shift=0):
    """y[j] = sum_i px[i] py[(j - i) mod D] on the count sketches px = psi(a, h1, s1), py = psi(v, h2, s2): the circular
    convolution as the sum it is.  A bucket that no (i, k) pair maps to is a sum of products with a zero factor: exactly 0.
    (``shift``: the off-by-one mutant (j - i + 1) mod D.)"""
    px = fusion.count_sketch(a, h1, s1, D)
    py = fusion.count_sketch(v, h2, s2, D)
    j = torch.arange(D)
    idx = (j[:, None] - j[None, :] + shift) % D                    # [j][i] -> (j - i) mod D
    return torch.einsum("...i,...ji->...j", px, py[..., idx])


def pool(a, v, h1, s1, h2, s2, D, shift=0):
    """the pooling of a case: the direct sum where D <= 260 (the sparse cases), else the FFT form"""
    if D <= 260:
        return mcb_direct(a, v, h1, s1, h2, s2, D, shift)
    if shift:
        return torch.roll(fusion.mcb(a, v, h1, s1, h2, s2, D), -shift, dims=-1)
    return fusion.mcb(a, v, h1, s1, h2, s2, D)


def reachable_buckets(h1, h2, D):
    """bool (D,): the buckets (h1[i] + h2[k]) mod D some input pair maps to"""
    hit = torch.zeros(D, dtype=torch.bool)
    hit[((h1[:, None] + h2[None, :]) % D).reshape(-1)] = True
    return hit


# ------------------------------------------------------------------------------------------ fusion: restatement, cases, reference
class _SignedSqrt(torch.autograd.Function):
    """sign(y) sqrt(|y| + eps); d/dy = 0.5 / sqrt(|y| + eps) for y != 0 and 0 at y == 0 (torch's sign and abs).
    ``keep_zero``: the mutant that does not zero the derivative at y == 0."""

    @staticmethod
    def forward(ctx, y, eps, keep_zero):
        r = torch.sqrt(torch.abs(y) + eps)
        ctx.save_for_backward(y, r)
        ctx.keep_zero = keep_zero
        return torch.sign(y) * r

    @staticmethod
    def backward(ctx, g):
        y, r = ctx.saved_tensors
        d = 0.5 / r
        if not ctx.keep_zero:
            d = d * (y != 0).to(y.dtype)
        return g * d, None, None


def post(y, w, b, rm, rv, eps, training, momentum, mutant=None):
    """``oracle.fusion.mcb_post`` with the BatchNorm written out (so that it can be mutated): y (B,T,D) ->
    (out (B,T,D), running_mean, running_var).  Equal to the oracle in float64 (tests/test_head_cpu.py)."""
    B, T, D = y.shape
    z = _SignedSqrt.apply(y, eps, mutant == "ssqrt_grad_at_zero")
    if mutant == "row_norm":
        n = z.detach().norm(dim=-1, keepdim=True).clamp_min(1e-30)
    else:           # accumulated in float64 like the kernel's: a float32 sum over 8.4 M elements (F3) is 2e-5 off by itself
        n = z.detach().double().norm().to(y.dtype)
    y2 = (z / n).reshape(B * T, D)
    if training:
        st = y2[:-1] if mutant == "bn_drops_last_row" else y2
        M = st.shape[0]
        mean = st.mean(0)
        var = ((st - mean) ** 2).mean(0)
        unb = var if mutant == "biased_running_var" else var * (M / (M - 1.0))
        rm = (1 - momentum) * rm + momentum * mean.detach()
        rv = (1 - momentum) * rv + momentum * unb.detach()
    else:
        mean, var = rm, rv
    out = (y2 - mean) / torch.sqrt(var + eps) * w + b
    return out.reshape(B, T, D), rm, rv


# rows = B x T.  Which code each case reaches (csrc/mcb.hip, csrc/bn_kernels.h; chunks(M, C): RL = 256 / (C / 4) row lanes,
# per = max(ceil(M / 512), 16 RL) rows per chunk rounded up to RL):
FUSION_CASES = {
    # two chunks of 16 and 1 rows: the second chunk's one U = 4 trip has three clamped rows
    "F1": dict(B=1, T=17, A=256, V=512, D=1024),
    # the c4 shape: 64 chunks; ssqrt_kernel and sum_partials over 1024 partial sums
    "F2": dict(B=64, T=16, A=256, V=512, D=1024),
    # 8208 rows: per = 17, 483 chunks, the last of 14 rows; every elementwise kernel runs its grid-stride loop
    "F3": dict(B=513, T=16, A=513, V=512, D=1024),
    # D % 256 != 0, Q = 65 (coefficients reloaded every iteration), RL = 3, two chunks; h1, h2 contain 0 and D - 1; exact zeros
    # (row 1 of F4 and F5 has an all-zero audio frame: its y is 0 at buckets the video does reach, the one place where the
    #  derivative of the signed square root at y == 0 decides a gradient -- d/d audio of that row)
    "F4": dict(B=53, T=1, A=33, V=20, D=260, hashes="edges", zero_audio_row=1),
    # every audio channel in bucket D - 1: one collision chain, the index wraps on every output
    "F4b": dict(B=53, T=1, A=33, V=20, D=260, hashes="collide"),
    # A + V < 256 and D < 256: most threads idle; almost every y is exactly 0
    "F5": dict(B=6, T=1, A=3, V=2, D=16, zero_audio_row=1),
    # Q = 3, RL = 85 (thread 255 idle), two chunks of 1360 and 40 rows
    "F6": dict(B=1400, T=1, A=5, V=7, D=12),
}


@functools.lru_cache(maxsize=None)
def fusion_inputs(name):
    """float32 inputs of a fusion case.  The running statistics are non-trivial and of the size the statistics of the
    L2-normalised tensor have (its elements are ~ 1 / sqrt(rows D)), so that eval mode is not output = bias and a wrong
    batch statistic is not lost below the old value's last bit."""
    c = FUSION_CASES[name]
    B, T, A, V, D = c["B"], c["T"], c["A"], c["V"], c["D"]
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + D)
    h1 = torch.from_numpy(rng.integers(0, D, A))
    h2 = torch.from_numpy(rng.integers(0, D, V))
    if c.get("hashes") == "edges":
        h1[0], h1[1], h2[-1], h2[-2] = 0, D - 1, 0, D - 1
    elif c.get("hashes") == "collide":
        h1[:] = D - 1
    rms2 = 1.0 / (B * T * D)
    a = _rand(rng, B, T, A)
    if "zero_audio_row" in c:
        a[c["zero_audio_row"]] = 0
    return types.SimpleNamespace(
        name=name, B=B, T=T, A=A, V=V, D=D, h1=h1, s1=_signs(rng, A), h2=h2, s2=_signs(rng, V),
        a=a, v=_rand(rng, B, T, V), G=_rand(rng, B, T, D),
        bn_w=_rand(rng, D) * 0.5 + 1.0, bn_b=_rand(rng, D),
        rm0=_rand(rng, D) * (0.3 * rms2 ** 0.5), rv0=(_rand(rng, D).abs() + 0.1) * rms2)


def fusion_pinned(y_impl, a, v, h1, s1, h2, s2, D, G, bn_w, bn_b, rm, rv, eps, training, momentum):
    """The float64 reference at the implementation's own pooled vector.  Step 1: ``oracle.fusion.mcb_post`` on
    ``y_impl.double()`` as a leaf, cotangent G: out, d bn_w, d bn_b, the updated running statistics and dY.  Step 2: dY through
    the float64 pooling of (a, v): d a, d v.  Also returns the float64 pooling itself (``y``)."""
    d = lambda t: t.detach().cpu().double()           # noqa: E731
    yl = d(y_impl).requires_grad_(True)
    w, b = d(bn_w).requires_grad_(True), d(bn_b).requires_grad_(True)
    rm, rv = d(rm).clone(), d(rv).clone()
    out = fusion.mcb_post(yl, w, b, rm, rv, eps, training, momentum)
    (out * d(G)).sum().backward()
    al, vl = d(a).requires_grad_(True), d(v).requires_grad_(True)
    y = pool(al, vl, h1, d(s1), h2, d(s2), D)
    (y * yl.grad).sum().backward()
    return dict(y=y.detach(), out=out.detach(), da=al.grad, dv=vl.grad, dw=w.grad, db=b.grad, rm=rm, rv=rv)


def fusion_fp32(inp, training, mutant=None):
    """The float32 CPU stand-in: ``pool`` (direct sum on the sparse cases) and ``post``, the restatement of
    ``oracle.fusion.mcb_post`` whose one sum over the whole tensor is accumulated in float64; with ``mutant`` one of them is made
    wrong.  Same signature and result as the GPU callable."""
    a, v = inp.a.clone().requires_grad_(True), inp.v.clone().requires_grad_(True)
    w, b = inp.bn_w.clone().requires_grad_(True), inp.bn_b.clone().requires_grad_(True)
    rm, rv = inp.rm0.clone(), inp.rv0.clone()
    y = pool(a, v, inp.h1, inp.s1, inp.h2, inp.s2, inp.D, shift=1 if mutant == "circular_off_by_one" else 0)
    out, rm, rv = post(y, w, b, rm, rv, EPS, training, MOMENTUM, mutant)
    (out * inp.G).sum().backward()
    return dict(y=y.detach(), out=out.detach(), da=a.grad, dv=v.grad, dw=w.grad, db=b.grad, rm=rm, rv=rv)


def check_fusion(impl, name, training, tag="gpu"):
    """``impl(inp, training)`` -> dict(y, out, da, dv, dw, db, rm, rv): y the implementation's own pooled vector (B,T,D), out the
    fusion's output, the gradients for cotangent ``inp.G`` and the running statistics after the call.

    Running statistics: next to the project's 1e-4 + 1e-5 |ref| they are held to 1e-5 max|ref| -- a hundred float32 ulps of
    the largest entry: the statistics of an L2-normalised tensor are ~ 1 / (rows D), where an absolute 1e-4 checks nothing,
    and what separates a float32 evaluation from float64 here is the rounding of y2 (6e-8 relative per element, averaged
    over the rows) and of the stored result."""
    inp = fusion_inputs(name)
    got = impl(inp, training)
    ref = fusion_pinned(got["y"], inp.a, inp.v, inp.h1, inp.s1, inp.h2, inp.s2, inp.D, inp.G, inp.bn_w, inp.bn_b, inp.rm0,
                        inp.rv0, EPS, training, MOMENTUM)
    t = "%s %s " % (name, "train" if training else "eval")
    report("fusion", t + "pooled y", got["y"], ref["y"], 1e-4, 1e-5, tag=tag)
    if inp.D <= 260:          # the direct sum's zeros are exact, and the signed square root is discontinuous there
        zero = ref["y"] == 0
        assert bool((got["y"].detach().cpu()[zero] == 0).all()), t + "pooled y is not exactly 0 where no input pair maps"
    report("fusion", t + "out", got["out"], ref["out"], 1e-4, tag=tag)
    for k, what in (("da", "d/d audio"), ("dv", "d/d video"), ("dw", "d/d bn weight"), ("db", "d/d bn bias")):
        report_grad("fusion", t + what, got[k], ref[k], tag=tag)
    for k, what in (("rm", "running_mean"), ("rv", "running_var")):
        report("fusion", t + what, got[k], ref[k], 1e-4, 1e-5, tag=tag)
        report("fusion", t + what + " (100 ulp)", got[k], ref[k], 1e-5 * float(ref[k].abs().max()), tag=tag)


# ------------------------------------------------------------------------------------------ raw pooling and sketch
POOLING_CASES = {
    "P2048": dict(rows=3, A=513, V=512, D=2048),         # the second pass of the j0 += 1024 loops
    "P1000": dict(rows=3, A=513, V=512, D=1000),         # D % 256 != 0 in the stand-alone kernels
}


@functools.lru_cache(maxsize=None)
def pooling_inputs(name):
    c = POOLING_CASES[name]
    rows, A, V, D = c["rows"], c["A"], c["V"], c["D"]
    rng = np.random.default_rng(D)
    return types.SimpleNamespace(name=name, rows=rows, A=A, V=V, D=D, h1=torch.from_numpy(rng.integers(0, D, A)),
                                 s1=_signs(rng, A), h2=torch.from_numpy(rng.integers(0, D, V)), s2=_signs(rng, V),
                                 a=_rand(rng, rows, A), v=_rand(rng, rows, V), G=_rand(rng, rows, D))


def pooling_fp32(inp, mutant=None):
    a, v = inp.a.clone().requires_grad_(True), inp.v.clone().requires_grad_(True)
    shift = 1 if mutant == "circular_off_by_one" else 0
    y = (torch.roll(fusion.mcb(a, v, inp.h1, inp.s1, inp.h2, inp.s2, inp.D), -shift, dims=-1))
    (y * inp.G).sum().backward()
    x = inp.a.clone().requires_grad_(True)
    sk = fusion.count_sketch(x, inp.h1, inp.s1, inp.D)
    (sk * inp.G).sum().backward()
    return dict(y=y.detach(), da=a.grad, dv=v.grad, sk=sk.detach(), dsk=x.grad)


@functools.lru_cache(maxsize=None)
def pooling_reference(name):
    """float64: the FFT form (dense inputs, D >= 1000) and the count sketch of ``a`` with (h1, s1), both with cotangent G"""
    inp = pooling_inputs(name)
    a, v = inp.a.double().requires_grad_(True), inp.v.double().requires_grad_(True)
    y = fusion.mcb(a, v, inp.h1, inp.s1.double(), inp.h2, inp.s2.double(), inp.D)
    (y * inp.G.double()).sum().backward()
    x = inp.a.double().requires_grad_(True)
    sk = fusion.count_sketch(x, inp.h1, inp.s1.double(), inp.D)
    (sk * inp.G.double()).sum().backward()
    return dict(y=y.detach(), da=a.grad, dv=v.grad, sk=sk.detach(), dsk=x.grad)


def check_pooling(impl, name, tag="gpu"):
    """``impl(inp)`` -> dict(y, da, dv, sk, dsk): CompactBilinearPooling's vector and input gradients, CountSketch's output
    and input gradient, all for cotangent ``inp.G``"""
    inp, ref = pooling_inputs(name), pooling_reference(name)
    got = impl(inp)
    report("pooling", name + " pooled y", got["y"], ref["y"], 1e-4, 1e-5, tag=tag)
    report_grad("pooling", name + " d/dx", got["da"], ref["da"], tag=tag)
    report_grad("pooling", name + " d/dy", got["dv"], ref["dv"], tag=tag)
    report("pooling", name + " sketch", got["sk"], ref["sk"], 1e-4, tag=tag)
    report_grad("pooling", name + " sketch d/dx", got["dsk"], ref["dsk"], tag=tag)


# ------------------------------------------------------------------------------------------ LSTM
def lstm_layer_mutable(x, lengths, w_ih, w_hh, b_ih, b_hh, mutant=None):
    """``oracle.head.lstm_layer`` with three places where it can be made wrong (equal to it without a mutant):
    ``state_runs_on``: the state keeps updating past the sequence's length; the layer's output IS its hidden state (the
    kernels read h_{t-1} back from y), so the padded output steps stop being zero;
    ``dh_last_unit``: the gradient that step t + 1 sends to h_t through the recurrent product is dropped for the last hidden
    unit; ``forget_grad_c``: the forget gate's gradient is taken with c_{t-2} instead of c_{t-1}."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    h = x.new_zeros(B, H)
    c = x.new_zeros(B, H)
    c_before = x.new_zeros(B, H)
    lengths = torch.as_tensor(lengths)
    outs = []
    for t in range(T):
        h_in = torch.cat([h[:, :-1], h[:, -1:].detach()], dim=1) if mutant == "dh_last_unit" else h
        gates = x[:, t] @ w_ih.t() + b_ih + h_in @ w_hh.t() + b_hh
        i, f, g, o = gates.chunk(4, dim=1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        if mutant == "forget_grad_c":      # the same value; d/df sees c_{t-2}
            c_new = f.detach() * c + (f - f.detach()) * c_before.detach() + i * g
        else:
            c_new = f * c + i * g
        h_new = o * torch.tanh(c_new)
        m = (t < lengths).to(x.dtype)[:, None]
        if mutant == "state_runs_on":
            m = torch.ones_like(m)
        c_before = c
        c = m * c_new + (1 - m) * c
        h = m * h_new + (1 - m) * h
        outs.append(m * h_new)
    return torch.stack(outs, dim=1)


# In = 40 unless stated; lengths ragged with lens[0] = T and at least one length of 1.  The kernel form of each case is
# what lstm_fwd_form / lstm_bwd_form below (csrc/lstm.hip's fwd_form / bwd_form, restated) give for it; the tests of
# tests/test_head_gpu.py name it, and test_case_lists_reach_what_they_claim (tests/test_head_cpu.py) holds them to it.
LSTM_CASES = {
    "L1": dict(B=16, H=256, T=60),
    "L1s": dict(B=16, H=256, T=60, no_persistent=True, same_as="L1"),
    "L2-T2": dict(B=32, H=256, T=2, lens="second_group_short"),
    "L2-T3": dict(B=32, H=256, T=3, lens="second_group_short"),
    "L3": dict(B=48, H=512, T=16, layers=2),
    "L3p": dict(B=32, H=512, T=16, layers=2),
    "L4": dict(B=64, H=1024, T=16),
    "L5": dict(B=128, H=64, T=60),
    "L6": dict(B=5, H=20, T=33, layers=2, In=7),
    "L7": dict(B=80, H=72, T=9),
    "L8-B16": dict(B=16, H=256, T=1),
    "L8-B3": dict(B=3, H=256, T=1),
    "L9": dict(B=16, H=256, T=5, misalign=True),
    "L1-T5": dict(B=16, H=256, T=5),
}
LSTM_SUBSETS = {            # what is frozen (of every layer); "x": the input needs no gradient (dx == nullptr)
    "x_without_grad": ("x",),
    "bias_ih_frozen": ("bias_ih",),
    "weight_hh_frozen": ("weight_hh",),
    "only_weight_ih": ("x", "weight_hh", "bias_ih", "bias_hh"),
}
LSTM_PARAMS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


# csrc/lstm.hip: step_form / fwd_form and bwd_form.  ``misalign``: weight_hh (or, forward, y) off a 16-byte boundary.
def lstm_fwd_form(B, T, H, misalign=False, lstm_no_fused_step=0, lstm_no_persistent=0):
    """(form, n, grid): ("PERSISTENT", NK, (H / 4, 1)) for steps 1 .. T-1 in one launch -- on a device that holds the grid;
    ("STEP", UB, grid) per step; ("GEMM", 0, None).  Step 0 is lstm_gates_fwd in every form, so T = 1 runs nothing else."""
    BG = min(B, 64)
    if not ((B in (16, 32) or (B % 64 == 0 and B <= 65535 * 64)) and H % (16 * (256 // BG)) == 0) or misalign \
            or lstm_no_fused_step:
        return "GEMM", 0, None
    if not lstm_no_persistent and B <= 64 and T > 1 and H % 64 == 0 and H // 64 in (4, 8, 16) and B * T * H * 4 < 1 << 31:
        return "PERSISTENT", H // 64, (H // 4, 1)
    UB = 4 if B >= 128 else 1
    return "STEP", UB, (H // (4 * UB), B // BG)


def lstm_bwd_form(B, T, H, misalign=False, lstm_no_fused_step=0):
    fused = (B <= 64 or H <= 64) and H % 4 == 0 and not misalign and not lstm_no_fused_step \
        and B * T * 4 * H < (1 << 29) - 64
    return "FUSED" if fused else "PLAIN"


@functools.lru_cache(maxsize=None)
def lstm_inputs(name):
    c = LSTM_CASES[name]
    B, H, T, layers, In = c["B"], c["H"], c["T"], c.get("layers", 1), c.get("In", 40)
    rng = np.random.default_rng(sum(map(ord, c.get("same_as", name))) * 104729 + B + H + T)
    if c.get("lens") == "second_group_short":       # sequences 16 .. 31 (the second group of 16) end after one step
        lens = [T] * 16 + [1] * (B - 16)
    else:
        lens = [int(n) for n in rng.integers(1, T + 1, B)]
        lens[0], lens[-1] = T, 1
    k = 1.0 / np.sqrt(H)                              # nn.LSTM's own initialisation
    sd = {}
    for l in range(layers):
        i = In if l == 0 else H
        for p, shape in (("weight_ih", (4 * H, i)), ("weight_hh", (4 * H, H)), ("bias_ih", (4 * H,)), ("bias_hh", (4 * H,))):
            sd["%s_l%d" % (p, l)] = torch.from_numpy(rng.uniform(-k, k, shape).astype(np.float32))
    return types.SimpleNamespace(name=name, B=B, H=H, T=T, In=In, layers=layers, lens=lens, sd=sd, x=_rand(rng, B, T, In),
                                 G=_rand(rng, B, T, H), no_persistent=bool(c.get("no_persistent")),
                                 misalign=bool(c.get("misalign")))


def _lstm_run(inp, dtype, frozen, mutant):
    sd = {k: t.to(dtype).clone().requires_grad_(k[:-3] not in frozen) for k, t in inp.sd.items()}
    x = inp.x.to(dtype).clone().requires_grad_("x" not in frozen)
    if mutant is None:
        y = head.lstm_stack(x, inp.lens, sd, "", inp.layers)
    else:
        y = x
        for l in range(inp.layers):
            y = lstm_layer_mutable(y, inp.lens, *(sd["%s_l%d" % (p, l)] for p in LSTM_PARAMS), mutant=mutant)
    (y * inp.G.to(dtype)).sum().backward()
    grads = {k: t.grad for k, t in sd.items()}
    grads["x"] = x.grad
    return y.detach(), grads


@functools.lru_cache(maxsize=None)
def lstm_reference(name):
    """``oracle.head.lstm_stack`` in float64: (y, {"x" / "<param>_l<layer>": gradient}) for cotangent G"""
    return _lstm_run(lstm_inputs(name), torch.float64, (), None)


def lstm_fp32(inp, frozen=(), mutant=None):
    """the float32 CPU stand-in (``oracle.head.lstm_stack``; with ``mutant``, ``lstm_layer_mutable``)"""
    return _lstm_run(inp, torch.float32, frozen, mutant)


def check_lstm(impl, name, frozen=(), tag="gpu"):
    """``impl(inp, frozen)`` -> (y, grads): grads maps "x" and "<param>_l<layer>" to the gradient for cotangent ``inp.G``, or
    to None for what ``frozen`` names ("x", "weight_ih", ... of every layer).  y, d x and every parameter gradient of every
    layer are compared; a frozen tensor must have no gradient."""
    inp = lstm_inputs(name)
    ref_y, ref_g = lstm_reference(name)
    y, grads = impl(inp, tuple(frozen))
    t = name + (" [frozen: %s] " % ",".join(frozen) if frozen else " ")
    report("lstm", t + "y", y, ref_y, 1e-4, tag=tag)
    assert set(grads) == set(ref_g), (sorted(grads), sorted(ref_g))
    for k in sorted(ref_g):
        if (k if k == "x" else k[:-3]) in frozen:
            assert grads[k] is None, t + k + " is frozen and has a gradient"
        else:
            assert grads[k] is not None, t + k + " has no gradient"
            report_grad("lstm", t + "d/d" + k, grads[k], ref_g[k], tag=tag)


# ------------------------------------------------------------------------------------------ losses
# logits uniform in [-8, 8] (Msat: [-40, 40]), targets in {0, 1}.  M1 is c2's 15 360 elements: the one workgroup of 1024
# threads walks its stride loop 15 times; M3 is one element beyond one trip.
MASKED_BCE_CASES = {
    "M1": dict(B=256, T=60, Y=1, lens="cycle"),          # lengths 1 .. 60
    "M2": dict(B=5, T=300, Y=3),
    "M3": dict(B=1, T=1025, Y=1),
    "Msat": dict(B=4, T=700, Y=1, span=40.0),
}


@functools.lru_cache(maxsize=None)
def masked_bce_inputs(name):
    c = MASKED_BCE_CASES[name]
    B, T, Y = c["B"], c["T"], c["Y"]
    rng = np.random.default_rng(B * 1000 + T + Y)
    span = c.get("span", 8.0)
    if c.get("lens") == "cycle":
        lens = [1 + b % T for b in range(B)]
    elif B == 1:
        lens = [T]
    else:
        lens = [int(n) for n in rng.integers(1, T + 1, B)]
        lens[0], lens[-1] = T, 1
    return types.SimpleNamespace(name=name, B=B, T=T, Y=Y, lens=lens, saturated="span" in c,
                                 logits=torch.from_numpy(rng.uniform(-span, span, (B, T, Y)).astype(np.float32)),
                                 targets=torch.from_numpy(rng.integers(0, 2, (B, T, Y)).astype(np.float32)))


def masked_bce_eval(inp, dtype, mutant=None):
    """(loss, d logits) of UPSTREAM * loss: ``oracle.head.batch_loss``; with ``mutant`` a restatement as one weighted sum in
    the kernel's flat element order (``norm_by_T``: normalised by T instead of len_b; ``first_1024_only``: the elements
    beyond flat index 1023 ignored; ``restated``: no mutation)"""
    r = inp.logits.to(dtype).clone().requires_grad_(True)
    x = inp.targets.to(dtype)
    if mutant is None:
        loss = head.batch_loss(r, x, inp.lens, EPS)
    else:
        lens = torch.tensor(inp.lens)
        live = (torch.arange(inp.T)[None, :, None] < lens[:, None, None]).to(dtype)
        s = torch.sigmoid(r)
        el = -(x * torch.log(s + EPS) + (1 - x) * torch.log(1 - s + EPS))
        denom = float(inp.T * inp.Y) if mutant == "norm_by_T" else (lens * inp.Y).to(dtype)[:, None, None]
        wgt = (live / denom).expand_as(el).reshape(-1).clone()
        if mutant == "first_1024_only":
            wgt[1024:] = 0
        loss = (el.reshape(-1) * wgt).sum()
    (loss * UPSTREAM).backward()
    return loss.detach(), r.grad


def masked_bce_fp32(inp, mutant=None):
    return masked_bce_eval(inp, torch.float32, mutant)


def check_masked_bce(impl, name, tag="gpu"):
    """``impl(inp)`` -> (loss, d logits of UPSTREAM * loss) against ``oracle.head.batch_loss`` in float64.

    Value: 1e-6 + 1e-5 |ref|.  Gradient: 1e-5 |ref| + atol element-wise (the gradients are ~ 1 / (len Y): the suite's
    absolute 1e-6 would check nothing).  atol = max(1e-9, 4 x what the float32 CPU oracle exceeds 1e-5 |ref| by on the same
    inputs): float32 rounds a sigmoid near 1 to 6e-8, which 1 - sigmoid carries as an absolute error of up to
    6e-8 UPSTREAM / (len Y) into the gradient -- 1e-9 is below that for the short sequences.  The saturated case (|r| up to
    40: 1 - sigmoid is quantised in float32, a float64 evaluation differs legitimately) takes for value and gradient 4 x the
    largest error of the float32 CPU oracle against the float64 one; 4 x because only the expf and the summation order
    differ between two float32 evaluations.  Both numbers go to the log."""
    inp = masked_bce_inputs(name)
    ref_loss, ref_g = masked_bce_eval(inp, torch.float64)
    o_loss, o_g = masked_bce_eval(inp, torch.float32)
    o_err_loss = float((o_loss.double() - ref_loss).abs())
    o_err_g = (o_g.double() - ref_g).abs()
    loss, g = impl(inp)
    loss = loss.detach().cpu().reshape(())
    if inp.saturated:
        b_loss, b_g = 4.0 * o_err_loss, 4.0 * float(o_err_g.max())
        if tag is not None:
            log_line("head %-5s bce      %s float32 oracle vs float64: value %.3e, gradient %.3e; bounds 4x: %.3e, %.3e"
                     % (tag, name, o_err_loss, float(o_err_g.max()), b_loss, b_g))
        assert b_loss > 0 and b_g > 0
        report("bce", name + " value (saturated)", loss, ref_loss, b_loss, tag=tag)
        report("bce", name + " d/d logits (saturated)", g, ref_g, b_g, tag=tag)
        return
    excess = float((o_err_g - 1e-5 * ref_g.abs()).max())
    atol = max(1e-9, 4.0 * excess)
    if tag is not None:
        log_line("head %-5s bce      %s float32 oracle exceeds 1e-5 |ref| by %.3e: gradient atol %.3e" % (tag, name, excess, atol))
    report("bce", name + " value", loss, ref_loss, 1e-6, 1e-5, tag=tag)
    report("bce", name + " d/d logits", g, ref_g, atol, 1e-5, tag=tag)


@functools.lru_cache(maxsize=None)
def bce_2classes_inputs():
    """rows = 1367, Y = 3: 4101 elements, five trips of the stride loop, the last of 5 elements; probabilities in (1e-6, 1)"""
    rng = np.random.default_rng(1367)
    p = lambda: torch.from_numpy(np.exp(rng.uniform(np.log(1e-6), 0.0, (1367, 3))).astype(np.float32)).clamp(1.1e-6, 1 - 1e-7)  # noqa: E731
    return types.SimpleNamespace(r1=p(), r2=p(), x=torch.from_numpy(rng.integers(0, 2, (1367, 3)).astype(np.float32)))


def bce_2classes_eval(inp, dtype, mutant=None):
    """(loss, d r1, d r2 of UPSTREAM * loss): ``oracle.head.bce_2classes``; ``first_1024_only``: a restatement as a flat sum that
    ignores the elements beyond flat index 1023"""
    r1, r2 = inp.r1.to(dtype).clone().requires_grad_(True), inp.r2.to(dtype).clone().requires_grad_(True)
    x = inp.x.to(dtype)
    if mutant is None:
        loss = head.bce_2classes(r1, r2, x, EPS)
    else:
        el = -(x * torch.log(r1 + EPS) + (1 - x) * torch.log(r2 + EPS)).reshape(-1)
        loss = (el[:1024] if mutant == "first_1024_only" else el).sum() / r1.shape[0]
    (loss * UPSTREAM).backward()
    return loss.detach(), r1.grad, r2.grad


def bce_2classes_fp32(inp, mutant=None):
    return bce_2classes_eval(inp, torch.float32, mutant)


def check_bce_2classes(impl, tag="gpu"):
    """``impl(inp)`` -> (loss, d r1, d r2 of UPSTREAM * loss) against ``oracle.head.bce_2classes`` in float64: the value at
    1e-6 + 1e-5 |ref|, the gradients (up to UPSTREAM / (1e-6 rows)) at the same bound, as test_bce_2classes_vs_reference"""
    inp = bce_2classes_inputs()
    ref_loss, ref_1, ref_2 = bce_2classes_eval(inp, torch.float64)
    loss, d1, d2 = impl(inp)
    report("bce2", "value", loss.detach().cpu().reshape(()), ref_loss, 1e-6, 1e-5, tag=tag)
    report("bce2", "d/d r1", d1, ref_1, 1e-6, 1e-5, tag=tag)
    report("bce2", "d/d r2", d2, ref_2, 1e-6, 1e-5, tag=tag)
