"""The oracle of the parameter-update tests: the optimiser step (``avvad_adam_step``, ``avvad.optim.FlatAdam``) and the small
kernels of csrc/misc.hip that share its launch geometry (``grid1``: at most 8192 workgroups of 256 threads, so 2 097 152 elements
per trip of a grid-stride loop, 8 388 608 floats per trip of the float4 Adam form).  It holds the cases, the seeded float32
inputs, the float64 references, the bounds and the assert / report helpers.  An assertion function takes the implementation
under test as an object: tests/test_update_gpu.py passes the HIP path, tests/test_update_cpu.py passes float32 CPU stand-ins
(the bounds must be within reach of a correct float32 evaluation of an independent operation order) and mutants (every bound
must be able to fail).

Adam.  The reference is a float64 numpy recurrence on the SAME float32 p0 and float32 gradients, with torch semantics:
m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps).  lr, the betas and eps are
rounded to float32 first (the entry point receives floats) and then widened; bc1 = 1 - b1^t and bc2 = 1 - b2^t are computed in
double from the float32 betas, as the entry point does.  Bound, for each of p, m and v, each gradient class and each checked
step: 4 x E32, where E32 is the largest deviation from the float64 reference, within the class, of a numpy float32 evaluation
of the same formula (``adam32``), floored at one float32 spacing of the class's max |q|.  The factor 4 covers fma contraction
and another operation order (the convention of tests/test_lip_gpu.py and tests/test_istft_gpu.py).  The three trajectories
(float64, float32 numpy, implementation) run independently from the same gradients, so accumulated rounding is inside E32.

The other kernels: copies, the transpose, the scaling by a device scalar and the row peak are exact (bit-equal to the float32
numpy / torch result); standardize, colsum and peak_normalize are compared with float64 at bounds derived where they are used.

Every comparison prints its figures; the worst error / bound ratio per case goes to the parity log of
tests/test_gpu_parity.py."""
import functools
import math
import os
import types

import numpy as np
import torch

from test_gpu_parity import OUT

LOG = os.path.join(OUT, "parity.log")              # the parity log ``test_gpu_parity._report`` appends to
U32 = 2.0 ** -24                                   # unit roundoff of float32
TRIP = 8192 * 256                                  # elements per trip of a grid1() grid-stride loop
TRIP4 = 4 * TRIP                                   # floats per trip of adam_kernel<4>
CANARY = 64                                        # floats before and after every buffer handed to a C entry point
CANARY_VALUE = 7.25


# ------------------------------------------------------------------------------------------ reporting
def log_line(msg):
    print(msg)
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(msg + "\n")
    except OSError:
        pass


def _np64(t):
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def report(name, got, ref, bound, tag="gpu"):
    """max over the elements of |got - ref| / bound must not exceed 1 (``bound``: a scalar or an array of ref's shape).  The
    figures are printed and, with a tag, appended to the parity log; tag None (the mutants) keeps them out of it."""
    got, ref = _np64(got), _np64(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(ref).all(), name + ": non-finite reference"
    err = np.abs(got - ref)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    ratio = float(q.max()) if q.size else 0.0
    msg = "update %-5s %-52s max|d|=%.3e  max|ref|=%.3e  max bound=%.3e  ratio=%.4f" % (
        tag or "", name, err.max() if err.size else 0.0, np.abs(ref).max() if ref.size else 0.0,
        bound.max() if bound.size else 0.0, ratio)
    if tag is not None:
        log_line(msg)
    assert np.isfinite(got).all(), name + ": non-finite values"
    assert ratio <= 1.0, msg
    return ratio


def bits(t):
    """the int32 bit patterns of a float32 tensor / array, as a numpy array (for bit-for-bit comparisons)"""
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.int32)


def assert_exact(name, got, ref, tag="gpu"):
    """bit-equal"""
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (name, g.shape, r.shape)
    bad = int((g != r).sum())
    msg = "update %-5s %-52s exact: %d of %d elements differ" % (tag or "", name, bad, g.size)
    if tag is not None:
        log_line(msg)
    assert bad == 0, msg


def with_canaries(x, off=0):
    """x (float32, 1-D numpy) inside a buffer with CANARY floats before and after it; ``off`` more floats in front move the
    payload off a 16-byte boundary.  -> (buffer, slice of the payload)"""
    lo = CANARY + off
    buf = np.full(lo + x.size + CANARY, CANARY_VALUE, dtype=np.float32)
    buf[lo:lo + x.size] = x
    return buf, slice(lo, lo + x.size)


def assert_canaries(name, buf, sl):
    b = bits(buf)
    c = np.float32(CANARY_VALUE).view(np.int32)
    assert bool((b[:sl.start] == c).all()), name + ": the floats in front of the buffer changed"
    assert bool((b[sl.stop:] == c).all()), name + ": the floats behind the buffer changed"


# ------------------------------------------------------------------------------------------ Adam: formula
def hyper32(lr, b1, b2, eps):
    """the hyperparameters as the entry point sees them: rounded to float32, then widened"""
    return tuple(float(np.float32(x)) for x in (lr, b1, b2, eps))


def bias_corrections(b1, b2, t):
    """in double from the (float32-valued) betas: csrc/misc.hip avvad_adam_step"""
    return 1.0 - b1 ** t, 1.0 - b2 ** t


def adam64(p, m, v, g, hp, t):
    """one step of the float64 reference, in place on float64 p, m, v; g float32"""
    lr, b1, b2, eps = hp
    bc1, bc2 = bias_corrections(b1, b2, t)
    g = g.astype(np.float64)
    m *= b1
    m += (1.0 - b1) * g
    v *= b2
    v += (1.0 - b2) * g * g
    p -= (lr / bc1) * (m / (np.sqrt(v) / math.sqrt(bc2) + eps))


MUTANTS = ("eps_inside_root", "bc2_without_root", "bc1_dropped")


def adam32(p, m, v, g, hp, t, mutant=None):
    """the same formula with every operation rounded to float32, in place on float32 p, m, v: what E32 is measured with, and
    (with ``mutant``) the stand-in that the bounds must reject"""
    f = np.float32
    lr, b1, b2, eps = (f(x) for x in hp)
    bc1, bc2 = bias_corrections(hp[1], hp[2], t)
    step_size = lr if mutant == "bc1_dropped" else lr / f(bc1)
    m[:] = b1 * m + (f(1) - b1) * g
    v[:] = b2 * v + (f(1) - b2) * g * g
    if mutant == "eps_inside_root":
        denom = np.sqrt(v / f(bc2) + eps)
    elif mutant == "bc2_without_root":
        denom = np.sqrt(v) / f(bc2) + eps
    else:
        denom = np.sqrt(v) / f(math.sqrt(bc2)) + eps
    upd = step_size * (m / denom)
    assert upd.dtype == np.float32 and m.dtype == np.float32 and v.dtype == np.float32
    p -= upd


class Numpy32:
    """``adam32`` as an implementation under test (the mutable float32 stand-in)"""

    def __init__(self, case, mutant=None):
        self.q = [case.p0.copy(), case.m0.copy(), case.v0.copy()]
        self.mutant = mutant

    def step(self, g, hp, t):
        adam32(*self.q, g, hp, t, self.mutant)

    def state(self):
        return self.q

    def finish(self):
        pass


# ------------------------------------------------------------------------------------------ Adam: cases
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8


def _normal(seed, k, n, scale=1.0):
    return (np.random.default_rng([seed, k]).standard_normal(n) * scale).astype(np.float32)


def _case(name, n, steps, check_at, classes, grad, hyper=None, first_step=1, m0=None, v0=None, off=0, zero_classes=(),
          p0=None, shapes=None, seed=0):
    hp = hyper32(LR, BETAS[0], BETAS[1], EPS)
    f32 = lambda x: np.zeros(n, dtype=np.float32) if x is None else np.ascontiguousarray(x, dtype=np.float32)   # noqa: E731
    assert classes[0][1].start == 0 and classes[-1][1].stop == n
    return types.SimpleNamespace(
        name=name, n=n, steps=steps, check_at=tuple(check_at), classes=classes, grad=grad, hyper=hyper or (lambda k: hp),
        first_step=first_step, p0=_normal(seed, 1000, n) if p0 is None else f32(p0), m0=f32(m0), v0=f32(v0), off=off,
        zero_classes=tuple(zero_classes), shapes=shapes)


def _blocks(n, names):
    """the column blocks of the gradient classes: ``names`` over [0, n), as equal as they come"""
    edges = [round(i * n / len(names)) for i in range(len(names) + 1)]
    return [(nm, slice(edges[i], edges[i + 1])) for i, nm in enumerate(names)]


A3_CLASSES = ("normal", "normal*1e-6", "normal*1e3", "constant", "alternating", "normal, zero from step 51", "zero")


def _a3_grad(seed, classes):
    sl = dict(classes)
    n = classes[-1][1].stop
    mag = np.abs(_normal(seed, 2000, n)) + np.float32(0.1)           # the alternating class: one magnitude per element

    def grad(k):                                                      # k = 0 .. steps - 1: the gradient of step k + 1
        z = _normal(seed, k, n)
        g = np.zeros(n, dtype=np.float32)
        g[sl["normal"]] = z[sl["normal"]]
        g[sl["normal*1e-6"]] = z[sl["normal*1e-6"]] * np.float32(1e-6)
        g[sl["normal*1e3"]] = z[sl["normal*1e3"]] * np.float32(1e3)
        g[sl["constant"]] = np.float32(0.37)
        g[sl["alternating"]] = mag[sl["alternating"]] * np.float32(1.0 if k % 2 == 0 else -1.0)
        if k < 50:
            g[sl["normal, zero from step 51"]] = z[sl["normal, zero from step 51"]]
        return g
    return grad


def flat_offsets(sizes):
    """FlatAdam's layout: every parameter starts at a multiple of 64 floats"""
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + (n + 63) // 64 * 64)
    return offs


C1_SHAPES = [(1,), (63,), (64,), (65,), (513,), (1000, 37), (8, 5)]      # the last one is handed over non-contiguous
C3_SHAPES = [(65,), (513,)]
C3_LRS = (1e-3, 3e-4, 3e-4, 2e-3)


def _param_case(name, shapes, steps, p0=None, hyper=None, seed=0):
    """one gradient class per parameter; the case's arrays are the parameters back to back, WITHOUT the layout's padding"""
    sizes = [int(np.prod(s)) for s in shapes]
    edges = np.concatenate([[0], np.cumsum(sizes)])
    classes = [("%d:%s" % (i, "x".join(map(str, s))), slice(int(edges[i]), int(edges[i + 1]))) for i, s in enumerate(shapes)]
    n = int(edges[-1])
    return _case(name, n, steps, range(1, steps + 1), classes, lambda k: _normal(seed, k, n), hyper=hyper, p0=p0,
                 shapes=[tuple(s) for s in shapes], seed=seed)


def trunk_parameters():
    """the parameters of the ResNet-18 trunk (avvad.nn.make_resnet18_trunk), seeded: 60 tensors (20 convolutions, 20 BatchNorm pairs), 11.2 M elements"""
    from avvad import nn as ann
    with torch.random.fork_rng():
        torch.manual_seed(2)
        trunk = ann.make_resnet18_trunk()
    return [p.detach() for p in trunk.parameters()]


@functools.lru_cache(maxsize=None)
def adam_case(name):
    if name == "A1":      # float4 form, two trips: a ragged second trip of 257 float4 and a scalar tail of 3
        n = TRIP4 + 4 * 257 + 3
        n4 = n // 4 * 4
        cl = [("trip 1", slice(0, TRIP4)), ("trip 2", slice(TRIP4, n4)), ("scalar tail", slice(n4, n))]
        return _case(name, n, 2, (1, 2), cl, lambda k: _normal(11, k, n), seed=11)
    if name == "A2":      # buffers one float off a 16-byte boundary: the scalar form, two trips, the second of 77
        n = TRIP + 77
        cl = [("trip 1", slice(0, TRIP)), ("trip 2", slice(TRIP, n))]
        return _case(name, n, 2, (1, 2), cl, lambda k: _normal(12, k, n), off=1, seed=12)
    if name == "A3":      # the long run: one column block per gradient class
        cl = _blocks(4096, A3_CLASSES)
        return _case(name, 4096, 200, (1, 2, 10, 200), cl, _a3_grad(13, cl), zero_classes=("zero",), seed=13)
    if name == "A4":      # other hyperparameters; lr drops from 1e-3 to 1e-4 at step 3
        cl = _blocks(4096, ("normal", "normal*1e-6"))
        scale = np.ones(4096, dtype=np.float32)
        scale[cl[1][1]] = 1e-6
        return _case(name, 4096, 5, range(1, 6), cl, lambda k: _normal(14, k, 4096) * scale,
                     hyper=lambda k: hyper32(1e-3 if k + 1 < 3 else 1e-4, 0.5, 0.9, 1e-3), seed=14)
    if name == "A4r":     # resume: steps 1000 .. 1002 from non-zero m and v; b2 = 0.999, so that bc2 = 1 - b2^1000 ~ 0.63
        cl = _blocks(4096, ("normal", "normal*1e-6"))
        scale = np.ones(4096, dtype=np.float32)
        scale[cl[1][1]] = 1e-6
        return _case(name, 4096, 3, (1000, 1001, 1002), cl, lambda k: _normal(15, k, 4096) * scale,
                     hyper=lambda k: hyper32(1e-3, 0.5, 0.999, 1e-3), first_step=1000,
                     m0=_normal(15, 3000, 4096, 0.1) * scale, v0=(_normal(15, 3001, 4096) ** 2 * 0.01 + 1e-4) * scale * scale,
                     seed=15)
    if name == "C1":
        return _param_case(name, C1_SHAPES, 3, seed=16)
    if name == "C2":
        ps = trunk_parameters()
        p0 = np.concatenate([p.reshape(-1).numpy() for p in ps]).astype(np.float32)
        return _param_case(name, [tuple(p.shape) for p in ps], 2, p0=p0, seed=17)
    if name == "C3":      # ``opt.lr`` changes between steps
        return _param_case(name, C3_SHAPES, len(C3_LRS), hyper=lambda k: hyper32(C3_LRS[k], BETAS[0], BETAS[1], EPS), seed=18)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------ Adam: the comparison
def spacing32(x):
    return float(np.spacing(np.float32(x)))


class AdamTrack:
    """The float64 reference and the float32 evaluation of a case, advanced in lockstep with the implementation under test,
    so that nothing but the current state is ever held (A1 and C2 are 8.4 M and 11.2 M elements)."""

    def __init__(self, case, tag="gpu"):
        self.case, self.tag = case, tag
        self.ref = [x.astype(np.float64) for x in (case.p0, case.m0, case.v0)]
        self.e32 = [x.copy() for x in (case.p0, case.m0, case.v0)]
        self.worst = (0.0, "nothing compared")
        self.failures = []

    def advance(self, g, hp, t):
        adam64(*self.ref, g, hp, t)
        adam32(*self.e32, g, hp, t)

    def compare(self, got, t):
        """p, m, v of the implementation after step t: per class against 4 x E32"""
        for q, (what, init) in enumerate((("p", self.case.p0), ("exp_avg", self.case.m0), ("exp_avg_sq", self.case.v0))):
            x = np.asarray(got[q])
            assert x.dtype == np.float32 and x.shape == (self.case.n,), (what, x.dtype, x.shape)
            assert np.isfinite(x).all(), "%s step %d: non-finite %s" % (self.case.name, t, what)
            for cname, sl in self.case.classes:
                r = self.ref[q][sl]
                e32 = max(float(np.abs(self.e32[q][sl] - r).max()), spacing32(np.abs(r).max()))
                err = float(np.abs(x[sl] - r).max())
                ratio = err / (4.0 * e32)
                where = "%s step %d %s [%s]" % (self.case.name, t, what, cname)
                line = "update %-5s adam %-44s max|d|=%.3e  E32=%.3e  bound=%.3e  ratio=%.4f" % (
                    self.tag or "", where, err, e32, 4.0 * e32, ratio)
                if self.tag is not None and len(self.case.classes) <= 8:
                    print(line)
                if ratio > self.worst[0]:
                    self.worst = (ratio, line)
                if ratio > 1.0:
                    self.failures.append(line)
                if cname in self.case.zero_classes and not np.array_equal(bits(x[sl]), bits(init[sl])):
                    self.failures.append("%s: not bit-identical to its initial values under a zero gradient" % where)

    def finish(self, check=True):
        """logs the case's worst ratio; -> that ratio"""
        if self.tag is not None:
            log_line("update %-5s adam %s WORST ratio=%.4f  (%s)" % (self.tag, self.case.name, self.worst[0],
                                                                    " ".join(self.worst[1].split()[3:])))
        if check:
            assert not self.failures, "\n".join(self.failures[:20])
        return self.worst[0]


def run_adam(case, make_impl, tag="gpu", check=True):
    """``make_impl(case)`` -> an object with ``step(g, hp, t)`` (g: float32 numpy (n,), hp = (lr, b1, b2, eps) as float32-valued
    floats, t the step number), ``state()`` -> (p, m, v) as float32 numpy (n,), and ``finish()`` (its own last assertions).
    -> the worst error / bound ratio."""
    impl = make_impl(case)
    track = AdamTrack(case, tag)
    for k in range(case.steps):
        t = case.first_step + k
        g, hp = case.grad(k), case.hyper(k)
        track.advance(g, hp, t)
        impl.step(g, hp, t)
        if t in case.check_at:
            track.compare(impl.state(), t)
    assert set(case.check_at) <= set(range(case.first_step, case.first_step + case.steps))
    impl.finish()
    return track.finish(check)


# ------------------------------------------------------------------------------------------ B1: copy_cols / ConcatColsFn
COPY_CASES = {"two trips": dict(lead=(4, 1025), wa=513, wb=2),          # 4100 rows x 513 columns > TRIP
              "one element": dict(lead=(1, 1), wa=1, wb=1)}


def _rand(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


def check_copy_cols(impl, name, tag="gpu"):
    """``impl.copy_cols(src, dst, rows, ncols, src_ld, src_off, dst_ld, dst_off)`` -> dst after the call (src, dst 1-D float32
    CPU tensors; dst includes everything the call must leave alone);  ``impl.concat(a, b, G)`` -> (cat, d a, d b) of
    ``ConcatColsFn`` with cotangent G."""
    c = COPY_CASES[name]
    rows, wa, wb = int(np.prod(c["lead"])), c["wa"], c["wb"]
    a_ld, a_off, dst_ld = wa + 3, 3, wa + wb + 1                    # strided source; the last column of dst is never written
    A, Bm = _rand(21, rows, a_ld), _rand(22, rows, wb)
    dst0 = torch.full((rows + 1, dst_ld), CANARY_VALUE)              # one more row behind the last
    exp = dst0.clone()
    exp[:rows, :wa] = A[:, a_off:]
    got = impl.copy_cols(A.reshape(-1), dst0.reshape(-1).clone(), rows, wa, a_ld, a_off, dst_ld, 0)
    assert_exact("copy_cols %s: %d columns from a strided source" % (name, wa), got, exp.reshape(-1), tag)
    exp[:rows, wa:wa + wb] = Bm
    got = impl.copy_cols(Bm.reshape(-1), got.clone(), rows, wb, wb, 0, dst_ld, wa)
    assert_exact("copy_cols %s: %d columns at a column offset" % (name, wb), got, exp.reshape(-1), tag)
    a, b = _rand(23, *c["lead"], wa), _rand(24, *c["lead"], wb)
    G = _rand(25, *c["lead"], wa + wb)
    cat, da, db = impl.concat(a, b, G)
    assert_exact("ConcatColsFn %s forward" % name, cat, torch.cat([a, b], -1), tag)
    assert_exact("ConcatColsFn %s d a" % name, da, G[..., :wa].contiguous(), tag)
    assert_exact("ConcatColsFn %s d b" % name, db, G[..., wa:].contiguous(), tag)


# ------------------------------------------------------------------------------------------ B2: scale_by_device_scalar
SCALE_SIZES = (TRIP + 5, 1)


def check_scale(impl, n, tag="gpu"):
    """``impl.scale(buf, lo, n, a)`` -> the buffer after x[lo:lo + n] *= a (a: a float32 value read from device memory)"""
    x = _rand(31, n).numpy()
    a = np.float32(0.3)
    buf, sl = with_canaries(x)
    got = impl.scale(torch.from_numpy(buf.copy()), sl.start, n, float(a))
    got = got.numpy() if isinstance(got, torch.Tensor) else got
    assert_canaries("scale n=%d" % n, got, sl)
    assert_exact("scale_by_device_scalar n=%d" % n, got[sl], x * a, tag)


# ------------------------------------------------------------------------------------------ B3: standardize
STANDARDIZE_CASES = {"per bin": dict(rows=4100, F=513, nstat=513),      # 4100 x 513 > TRIP
                     "scalar": dict(rows=470, F=4489, nstat=1)}         # 470 frames of 67 x 67 > TRIP
STD_EPS = 1e-8


@functools.lru_cache(maxsize=None)
def standardize_inputs(name):
    """the per-bin case gives bin 7 a standard deviation of exactly 0: there ``eps`` alone is the divisor"""
    c = STANDARDIZE_CASES[name]
    rows, F, nstat = c["rows"], c["F"], c["nstat"]
    x = _rand(41, rows, F)
    if nstat == 1:
        mean, std = torch.tensor([[0.4]]), torch.tensor([[2.5]])
    else:
        mean, std = _rand(42, F, 1), _rand(43, F, 1).abs() + 0.5
        std[7] = 0.0
    return x, mean, std


def standardize64(x, mean, std, eps=STD_EPS):
    """float64; eps rounded to float32 first, as the entry point receives it"""
    return (x.double() - mean.double().reshape(-1)) / (std.double().reshape(-1) + float(np.float32(eps)))


def check_standardize(impl, name, tag="gpu"):
    """``impl.standardize(x, mean, std, eps)`` against float64 at 1e-6 + 1e-6 |ref|, the bound of
    test_input_standardisation_in_the_train_loop and test_standardize_peak_normalize_and_peak"""
    x, mean, std = standardize_inputs(name)
    ref = standardize64(x, mean, std)
    got = impl.standardize(x, mean, std, STD_EPS)
    report("standardize %s (%d x %d)" % (name, x.shape[0], x.shape[1]), got, ref, 1e-6 + 1e-6 * ref.abs().numpy(), tag)
    if name == "per bin":
        assert float(ref[:, 7].abs().max()) > 1e7               # eps decided that column
        report("standardize %s, the std = 0 bin" % name, got[:, 7], ref[:, 7], 1e-6 + 1e-6 * ref[:, 7].abs().numpy(), tag)


# ------------------------------------------------------------------------------------------ B4: transpose
TRANSPOSE_SHAPES = ((3, 33, 65), (2, 31, 1), (2, 1, 40), (1, 32, 32), (1, 1, 1))


def check_transpose(impl, shape, tag="gpu"):
    """``impl.transpose(buf, lo, B, C, T)`` -> the output buffer (canaries around B*T*C floats at lo) of avvad_transpose_last2;
    ``impl.transpose_fn(x, G)`` -> (y, d x) of ``TransposeLast2Fn`` with cotangent G"""
    B, Cc, T = shape
    x = _rand(51, B, Cc, T)
    exp = x.transpose(1, 2).contiguous()
    buf, sl = with_canaries(np.zeros(x.numel(), dtype=np.float32))
    got = impl.transpose(x, torch.from_numpy(buf), sl.start, B, Cc, T)
    got = got.numpy() if isinstance(got, torch.Tensor) else got
    assert_canaries("transpose %s" % (shape,), got, sl)
    assert_exact("transpose_last2 %dx%dx%d" % shape, got[sl], exp.reshape(-1), tag)
    G = _rand(52, B, T, Cc)
    y, dx = impl.transpose_fn(x, G)
    assert_exact("TransposeLast2Fn %dx%dx%d forward" % shape, y, exp, tag)
    assert_exact("TransposeLast2Fn %dx%dx%d d x" % shape, dx, G.transpose(1, 2).contiguous(), tag)


# ------------------------------------------------------------------------------------------ B5: colsum
COLSUM_ROWS = (1, 3, 4, 5, 15360)
COLSUM_COLS = (1, 64, 65, 513)


def check_colsum(impl, rows, cols, tag="gpu"):
    """``impl.colsum(X, buf, lo)`` -> the buffer after out[c] += sum_r X[r][c] on the ``cols`` floats at lo.

    The kernel gives each column to 4 threads; thread j adds rows j, j + 4, ... in order (ceil(rows / 4) additions at most,
    each within 2^-24 of its partial sum, which never exceeds sum_r |X[r][c]|), then ((s0 + s1) + s2) + s3 and the addition to
    the old value of out: 4 more roundings of sums within sum_r |X[r][c]| + |out0[c]|.  Hence
    |error| <= (ceil(rows / 4) + 4) 2^-24 sum_r |X[r][c]| + 2^-24 |out0[c]|."""
    X = _rand(61 + rows + cols, rows, cols)
    out0 = _rand(62, cols).numpy() * np.float32(3.0) + np.float32(0.5)
    assert bool((out0 != 0).all())
    buf, sl = with_canaries(out0)
    got = impl.colsum(X, torch.from_numpy(buf.copy()), sl.start)
    got = got.numpy() if isinstance(got, torch.Tensor) else got
    assert_canaries("colsum %dx%d" % (rows, cols), got, sl)
    X64 = X.double().numpy()
    ref = out0.astype(np.float64) + X64.sum(0)
    bound = (math.ceil(rows / 4) + 4) * U32 * np.abs(X64).sum(0) + U32 * np.abs(out0.astype(np.float64))
    report("colsum_acc %d x %d" % (rows, cols), got[sl], ref, bound, tag)


# ------------------------------------------------------------------------------------------ B6: peak / peak_normalize
PEAK_LENGTHS = (1, 1023, 1024, 1025, 3000)


def check_peak(impl, L, tag="gpu"):
    """B = 3: the peak is the first sample of row 0, the last sample of row 1 and a negative value in the middle of row 2.
    ``impl.peak(w)`` is exact; ``impl.peak_normalize(w)`` is one float32 division of values that end up within [-1, 1]:
    within 2^-23 |q| of the float64 quotient q (a correctly rounded division is within 2^-24 |q|; a reciprocal and a
    multiplication is one more rounding)."""
    w = _rand(71 + L, 3, L, scale=0.3).clamp(-0.9, 0.9)
    w[0, 0], w[1, L - 1], w[2, L // 2] = 1.25, 1.5, -1.75
    exp = torch.tensor([1.25, 1.5, 1.75])
    assert torch.equal(w.abs().max(dim=1).values, exp)
    assert_exact("peak L=%d" % L, impl.peak(w), exp, tag)
    q = w.double() / exp.double()[:, None]
    report("peak_normalize L=%d" % L, impl.peak_normalize(w), q, 2.0 ** -23 * q.abs().numpy(), tag)
