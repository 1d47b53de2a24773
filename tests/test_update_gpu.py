"""The step that writes the parameters, on the GPU: ``avvad_adam_step`` through the C ABI at the sizes where its grid-stride
loops take a second trip, ``avvad.optim.FlatAdam`` on the layouts training uses, and the small kernels of csrc/misc.hip around
it (copy_cols, scale_by_device_scalar, standardize, transpose_last2, colsum_acc, peak / peak_normalize) -- against the float64
references and exact results of tests/update_ref.py.  The cases, bounds and assertion functions are update_ref's;
tests/test_update_cpu.py runs the same cases with float32 CPU stand-ins in the place of the HIP path."""
import ctypes as C

import numpy as np
import pytest
import torch

import update_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAG = "gpu"


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from avvad import _lib as L
    return L, L.lib()


def _dev(t):
    return (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV)


# ------------------------------------------------------------------------------------------ A: avvad_adam_step
class HipAdam:
    """p, g, m, v each inside a buffer of its own with 64 canary floats on both sides; ``case.off`` floats more in front put
    all four one float off a 16-byte boundary"""

    def __init__(self, case):
        self.case = case
        self.bufs, self.views = [], []
        for x in (case.p0, np.zeros(case.n, dtype=np.float32), case.m0, case.v0):
            buf, sl = R.with_canaries(x, case.off)
            buf = _dev(buf)
            self.bufs.append(buf)
            self.views.append(buf[sl.start:sl.stop])
        self.sl = sl
        for v in self.views:
            assert v.data_ptr() % 16 == 4 * case.off and v.numel() == case.n

    def step(self, g, hp, t):
        L, lib = _lib()
        p, gr, m, v = self.views
        gr.copy_(_dev(g))
        L.check(lib.avvad_adam_step(L.ptr(p), L.ptr(gr), L.ptr(m), L.ptr(v), self.case.n, *hp, t, _stream()), "avvad_adam_step")
        self.g = g

    def state(self):
        p, _, m, v = self.views
        return [x.cpu().numpy() for x in (p, m, v)]

    def finish(self):
        for name, buf in zip(("param", "grad", "exp_avg", "exp_avg_sq"), self.bufs):
            R.assert_canaries("%s %s" % (self.case.name, name), buf, self.sl)
        assert np.array_equal(R.bits(self.views[1]), R.bits(self.g)), "the gradient is an input: it must not change"


@pytest.mark.parametrize("name", ["A1", "A2", "A3", "A4", "A4r"])
def test_adam_step(name):
    """A1: the float4 form over two trips, a ragged second one and a scalar tail of 3.  A2: the scalar form (buffers one float
    off alignment) over two trips.  A3: 200 steps, one column block per gradient class, checked at steps 1, 2, 10 and 200; the
    all-zero class stays bit-identical.  A4: betas (0.5, 0.9), eps 1e-3, lr dropping at step 3.  A4r: steps 1000 .. 1002 from
    non-zero m and v.  p, exp_avg and exp_avg_sq against float64 at 4 x E32 per class; canaries around all four buffers."""
    R.run_adam(R.adam_case(name), HipAdam, tag=TAG)


def test_adam_step_refusals():
    """step = 0 is refused with nothing written; n = 0 returns OK with nothing written"""
    L, lib = _lib()
    n = 1001
    vals = [R._rand(80 + i, n).numpy() for i in range(4)]
    vals[3] = np.abs(vals[3])
    bufs = [_dev(R.with_canaries(x)[0]) for x in vals]
    before = [b.clone() for b in bufs]
    p, g, m, v = (b[R.CANARY:R.CANARY + n] for b in bufs)
    hp = R.hyper32(R.LR, R.BETAS[0], R.BETAS[1], R.EPS)
    assert lib.avvad_adam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, *hp, 0, _stream()) == -1          # AVVAD_EINVAL
    assert lib.avvad_adam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, *hp, -3, _stream()) == -1
    assert lib.avvad_adam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), 0, *hp, 1, _stream()) == 0           # AVVAD_OK
    torch.cuda.synchronize()
    for b, b0 in zip(bufs, before):
        assert np.array_equal(R.bits(b), R.bits(b0))


# ------------------------------------------------------------------------------------------ B: the other misc.hip kernels
class Hip:
    def copy_cols(self, src, dst, rows, ncols, src_ld, src_off, dst_ld, dst_off):
        L, lib = _lib()
        s, d = _dev(src), _dev(dst)
        L.check(lib.avvad_copy_cols(L.ptr(s), L.ptr(d), rows, ncols, src_ld, src_off, dst_ld, dst_off, _stream()), "avvad_copy_cols")
        return d.cpu()

    def concat(self, a, b, G):
        from avvad import ops
        a, b = _dev(a).requires_grad_(True), _dev(b).requires_grad_(True)
        y = ops.ConcatColsFn.apply(a, b)
        (y * _dev(G)).sum().backward()
        return y.detach(), a.grad, b.grad

    def scale(self, buf, lo, n, a):
        L, lib = _lib()
        d, s = _dev(buf), torch.tensor([a], dtype=torch.float32, device=DEV)
        L.check(lib.avvad_scale_by_device_scalar(L.ptr(d[lo:lo + n]), L.ptr(s), n, _stream()), "avvad_scale_by_device_scalar")
        return d.cpu()

    def standardize(self, x, mean, std, eps):
        from avvad import ops
        return ops.standardize(_dev(x), _dev(mean), _dev(std), eps)

    def transpose(self, x, buf, lo, B, Cc, T):
        L, lib = _lib()
        xd, d = _dev(x), _dev(buf)
        L.check(lib.avvad_transpose_last2(L.ptr(xd), L.ptr(d[lo:lo + xd.numel()]), B, Cc, T, _stream()), "avvad_transpose_last2")
        return d.cpu()

    def transpose_fn(self, x, G):
        from avvad import ops
        x = _dev(x).requires_grad_(True)
        y = ops.TransposeLast2Fn.apply(x)
        (y * _dev(G)).sum().backward()
        return y.detach(), x.grad

    def colsum(self, X, buf, lo):
        L, lib = _lib()
        Xd, d = _dev(X), _dev(buf)
        L.check(lib.avvad_colsum_acc(L.ptr(Xd), X.shape[0], X.shape[1], L.ptr(d[lo:lo + X.shape[1]]), _stream()), "avvad_colsum_acc")
        return d.cpu()

    def peak(self, w):
        from avvad import ops
        return ops.peak(_dev(w))

    def peak_normalize(self, w):
        from avvad import ops
        return ops.peak_normalize(_dev(w))


@pytest.mark.parametrize("name", list(R.COPY_CASES))
def test_copy_cols_and_concat(name):
    """avvad_copy_cols with a strided source and a column offset into a wider destination, and ConcatColsFn forward and
    backward: exact.  4100 rows x 513 columns take a second trip of the grid-stride loop; (1, 1) x 1 row is the smallest."""
    R.check_copy_cols(Hip(), name, tag=TAG)


@pytest.mark.parametrize("n", R.SCALE_SIZES)
def test_scale_by_device_scalar(n):
    """n = 2 097 152 + 5 (a second trip of 5) and n = 1: exact, nothing written around the buffer"""
    R.check_scale(Hip(), n, tag=TAG)


@pytest.mark.parametrize("name", list(R.STANDARDIZE_CASES))
def test_standardize(name):
    """per-bin statistics at 4100 x 513 (one bin with std = 0: eps is the divisor) and scalar statistics at 470 frames of
    67 x 67, both beyond one trip, against float64"""
    R.check_standardize(Hip(), name, tag=TAG)


@pytest.mark.parametrize("shape", R.TRANSPOSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_transpose_last2(shape):
    """avvad_transpose_last2 and TransposeLast2Fn forward and backward: exact; partial 32 x 32 tiles on both axes, T = 1,
    C = 1, one full tile, one element"""
    R.check_transpose(Hip(), shape, tag=TAG)


@pytest.mark.parametrize("cols", R.COLSUM_COLS)
@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_colsum_acc(rows, cols):
    """out[c] += sum_r X[r][c] on a non-zero ``out``: fewer rows than the 4 row lanes, one more, the c2 row count; one column,
    one 64-column workgroup, one column more, the 513 bins -- against float64 at the bound of the kernel's summation order"""
    R.check_colsum(Hip(), rows, cols, tag=TAG)


@pytest.mark.parametrize("L", R.PEAK_LENGTHS)
def test_peak_and_peak_normalize(L):
    """one sample, one short of / exactly / one beyond the 1024 threads of the row's workgroup, three trips; the peak first,
    last and negative"""
    R.check_peak(Hip(), L, tag=TAG)


# ------------------------------------------------------------------------------------------ C: FlatAdam
class FlatAdamImpl:
    """FlatAdam over one Parameter per class of the case; the gradients arrive through ``p.grad.copy_`` and ``opt.lr`` is set
    before every step.  ``state()`` gathers p from the parameters themselves and m, v from the flat buffers at ``opt.offsets``."""

    def __init__(self, case, params=None, opt=None):
        self.case = case
        self.params = params or [torch.nn.Parameter(_dev(case.p0[sl].reshape(shape)))
                                 for (_, sl), shape in zip(case.classes, case.shapes)]
        self.opt = opt

    def step(self, g, hp, t):
        from avvad.optim import FlatAdam
        lr, b1, b2, eps = hp
        if self.opt is None:
            self.opt = FlatAdam(self.params, lr=lr, betas=(b1, b2), eps=eps)
        assert self.opt.t == t - 1 and (self.opt.betas, self.opt.eps) == ((b1, b2), eps)
        self.opt.lr = lr
        for p, (_, sl) in zip(self.opt.params, self.case.classes):
            p.grad.copy_(_dev(g[sl].reshape(tuple(p.shape))))
        self.opt.step()

    def state(self):
        o = self.opt
        p = torch.cat([q.detach().reshape(-1) for q in o.params])
        m, v = (torch.cat([buf[s:s + q.numel()] for q, s in zip(o.params, o.offsets)]) for buf in (o.exp_avg, o.exp_avg_sq))
        return [x.cpu().numpy() for x in (p, m, v)]

    def padding(self):
        """bool mask over the flat buffers: the slots between the parameters"""
        o = self.opt
        pad = torch.ones(o.flat.numel(), dtype=torch.bool, device=o.flat.device)
        for q, s in zip(o.params, o.offsets):
            pad[s:s + q.numel()] = False
        return pad

    def finish(self):
        o = self.opt
        pad = self.padding()
        for name in ("flat", "flat_grad", "exp_avg", "exp_avg_sq"):
            assert int(torch.count_nonzero(getattr(o, name)[pad].view(torch.int32))) == 0, "%s: padding of %s is not bit-zero" % (
                self.case.name, name)


def test_flat_adam_layout():
    """C1: sizes 1, 63, 64, 65, 513, a 1000 x 37 tensor and a non-contiguous one, a frozen parameter in the middle, one
    parameter that already holds a gradient.  Values and the existing gradient are carried over bit for bit, every parameter
    and its gradient are views at flat base + 4 offset with offsets in multiples of 64, the frozen parameter is untouched;
    after three steps the padding of all four buffers is bit-zero and every parameter meets the bound of the C ABI cases;
    dist.flat_views lays the same list out at the same offsets."""
    from avvad import dist
    from avvad.optim import FlatAdam
    case = R.adam_case("C1")
    vals = [torch.from_numpy(case.p0[sl].reshape(shape)) for (_, sl), shape in zip(case.classes, case.shapes)]
    trainable = [torch.nn.Parameter(_dev(v)) for v in vals[:-1]]
    nc = _dev(vals[-1]).t().contiguous().t()                      # the values of vals[-1], column-major in memory
    assert not nc.is_contiguous() and torch.equal(nc.cpu(), vals[-1])
    trainable.append(torch.nn.Parameter(nc))
    assert not trainable[-1].is_contiguous()
    g0 = R._rand(91, 513)
    trainable[4].grad = _dev(g0)                                  # the 513-element parameter arrives with a gradient
    frozen_vals = R._rand(92, 77)
    frozen = torch.nn.Parameter(_dev(frozen_vals), requires_grad=False)
    frozen_ptr = frozen.data_ptr()
    plist = trainable[:3] + [frozen] + trainable[3:]
    hp = case.hyper(0)
    opt = FlatAdam(plist, lr=hp[0], betas=hp[1:3], eps=hp[3])
    assert len(opt.params) == len(trainable) and all(p is q for p, q in zip(opt.params, trainable))
    assert opt.offsets == R.flat_offsets([v.numel() for v in vals]) and opt.flat.numel() == opt.offsets[-1]
    for i, (p, v, o) in enumerate(zip(trainable, vals, opt.offsets)):
        assert o % 64 == 0
        assert p.data_ptr() == opt.flat.data_ptr() + 4 * o and p.grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * o, i
        assert p.is_contiguous() and p.grad.is_contiguous() and p.shape == v.shape == p.grad.shape
        assert np.array_equal(R.bits(p), R.bits(v)), "parameter %d changed on its way into the flat buffer" % i
        assert np.array_equal(R.bits(opt.flat[o:o + v.numel()]), R.bits(v.reshape(-1)))
        want_g = g0 if i == 4 else torch.zeros_like(v)
        assert np.array_equal(R.bits(p.grad), R.bits(want_g)), "gradient %d" % i
    assert frozen.data_ptr() == frozen_ptr and frozen.grad is None and np.array_equal(R.bits(frozen), R.bits(frozen_vals))
    impl = FlatAdamImpl(case, opt=opt)
    impl.finish()                                                 # the padding is zero before the first step as well
    R.run_adam(case, lambda c: impl, tag=TAG)
    assert np.array_equal(R.bits(frozen), R.bits(frozen_vals)) and frozen.data_ptr() == frozen_ptr
    flat, offs = dist.flat_views(plist)                           # last: it re-homes every .grad
    assert offs == opt.offsets and flat.numel() == opt.flat.numel()


def test_flat_adam_training_layout():
    """C2: the parameters of the ResNet-18 trunk (11.2 M elements in 60 tensors, never run) in one flat buffer beyond one trip
    of the float4 form; seeded gradients through ``copy_``, two steps, every parameter at the bound of the C ABI cases"""
    case = R.adam_case("C2")
    impl = FlatAdamImpl(case)
    R.run_adam(case, lambda c: impl, tag=TAG)
    assert impl.opt.flat.numel() > 8388608 and impl.opt.t == 2


def test_flat_adam_honours_lr_changes():
    """C3: ``opt.lr`` set to 1e-3, 3e-4, 3e-4, 2e-3 before the four steps; the reference takes the same schedule"""
    case = R.adam_case("C3")
    assert len({case.hyper(k)[0] for k in range(case.steps)}) == 3
    R.run_adam(case, FlatAdamImpl, tag=TAG)


@pytest.mark.parametrize("how", ["set_to_none", "replaced"])
def test_flat_adam_refuses_a_stray_gradient(how):
    """C4: once ``.grad`` of a parameter is None or another tensor, backward fills a gradient OUTSIDE the flat buffer, and a step
    would apply the flat buffer's zeros in its place.  ``step()`` raises AvvadError naming the parameter before any launch:
    ``opt.t`` and all four buffers are unchanged.  After ``zero_grad()`` (which re-attaches the view) the run continues and
    matches the float64 reference."""
    from avvad import AvvadError
    from avvad.optim import FlatAdam
    case = R.adam_case("C3")
    impl = FlatAdamImpl(case)
    track = R.AdamTrack(case, TAG)
    g, hp = case.grad(0), case.hyper(0)
    track.advance(g, hp, 1)
    impl.step(g, hp, 1)
    opt, ps = impl.opt, impl.opt.params
    assert isinstance(opt, FlatAdam)
    opt.zero_grad()
    if how == "set_to_none":
        ps[1].grad = None
    else:
        ps[1].grad = torch.zeros_like(ps[1])
    w = [_dev(R._rand(95 + i, *p.shape)) for i, p in enumerate(ps)]
    sum((p * wi).sum() for p, wi in zip(ps, w)).backward()        # a backward that fills the stray gradient
    assert torch.equal(ps[1].grad, w[1]) and ps[1].grad.data_ptr() != opt.flat_grad.data_ptr() + 4 * opt.offsets[1]
    assert torch.equal(ps[0].grad, w[0]) and ps[0].grad.data_ptr() == opt.flat_grad.data_ptr()
    names = ("flat", "flat_grad", "exp_avg", "exp_avg_sq")
    before = [getattr(opt, nm).clone() for nm in names]
    with pytest.raises(AvvadError, match=r"parameter 1 \(shape \(513,\)\)"):
        opt.step()
    assert opt.t == 1
    for nm, b in zip(names, before):
        assert np.array_equal(R.bits(getattr(opt, nm)), R.bits(b)), nm + " changed in a refused step"
    opt.zero_grad()
    assert all(p.grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * o for p, o in zip(ps, opt.offsets))
    assert int(torch.count_nonzero(opt.flat_grad)) == 0
    for k in range(1, case.steps):
        g, hp = case.grad(k), case.hyper(k)
        track.advance(g, hp, k + 1)
        impl.step(g, hp, k + 1)
        track.compare(impl.state(), k + 1)
    impl.finish()
    track.finish()
