"""CPU tests of the parameter-update oracle (tests/update_ref.py): the cases reach what they claim, the float64 recurrence is
torch's Adam, every case of tests/test_update_gpu.py runs with a float32 CPU stand-in in the place of the HIP path (the bounds
are within reach of a correct float32 evaluation in ANOTHER operation order: torch.optim.Adam and torch's own kernels), and
three mutants of the float32 formula fail the bound (every bound can fail)."""
import math

import numpy as np
import pytest
import torch

import update_ref as R

TAG = "cpu32"


# ------------------------------------------------------------------------------------------ the cases reach what they claim
def test_case_lists_reach_what_they_claim():
    a1, a2 = R.adam_case("A1"), R.adam_case("A2")
    assert R.TRIP == 2097152 and R.TRIP4 == 8388608
    assert a1.n == 8388608 + 4 * 257 + 3 and a1.off == 0 and a1.n % 4 == 3 and a1.n // 4 > R.TRIP    # second float4 trip + tail
    assert a2.n == 2097152 + 77 and a2.off == 1                                                       # second scalar trip
    a3 = R.adam_case("A3")
    assert a3.n == 4096 and a3.steps == 200 and a3.check_at == (1, 2, 10, 200)
    assert [c for c, _ in a3.classes] == list(R.A3_CLASSES) and len(a3.classes) == 7
    sl = dict(a3.classes)
    g0, g1, g50 = a3.grad(0), a3.grad(1), a3.grad(50)
    assert 1e-7 < np.abs(g0[sl["normal*1e-6"]]).max() < 1e-5 and 1e2 < np.abs(g0[sl["normal*1e3"]]).max() < 1e4
    assert np.ptp(g0[sl["constant"]]) == 0 and np.array_equal(g0[sl["constant"]], g1[sl["constant"]])
    assert np.array_equal(g0[sl["alternating"]], -g1[sl["alternating"]]) and bool((g0[sl["alternating"]] != 0).all())
    assert a3.grad(49)[sl["normal, zero from step 51"]].any() and not g50[sl["normal, zero from step 51"]].any()
    assert not any(a3.grad(k)[sl["zero"]].any() for k in (0, 1, 199))
    a4, a4r = R.adam_case("A4"), R.adam_case("A4r")
    f = lambda x: float(np.float32(x))         # noqa: E731
    assert a4.hyper(1) == (f(1e-3), 0.5, f(0.9), f(1e-3)) and a4.hyper(2)[0] == f(1e-4)              # lr drops AT step 3
    assert a4r.first_step == 1000 and a4r.m0.all() and (a4r.v0 > 0).all()
    assert abs(R.bias_corrections(*a4r.hyper(0)[1:3], 1000)[1] - 0.63) < 0.01
    assert 4100 * 513 > R.TRIP and 470 * 4489 > R.TRIP and min(R.SCALE_SIZES) == 1 and max(R.SCALE_SIZES) == R.TRIP + 5
    c2 = R.adam_case("C2")
    assert len(c2.shapes) == 60 and R.flat_offsets([int(np.prod(s)) for s in c2.shapes])[-1] > 8388608


def test_flat_views_lays_the_parameters_out_like_the_optimiser():
    """``dist.flat_views`` (the bucket reducer is constructed on its offsets) and FlatAdam's layout as ``flat_offsets`` restates
    it, on the C1 list with a frozen parameter in the middle and on the trunk's parameters"""
    from avvad import dist
    for shapes in (R.C1_SHAPES, R.adam_case("C2").shapes):
        ps = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
        ps.insert(3, torch.nn.Parameter(torch.zeros(77), requires_grad=False))
        flat, offs = dist.flat_views(ps)
        assert offs == R.flat_offsets([int(np.prod(s)) for s in shapes]) and flat.numel() == offs[-1]
        assert all(o % 64 == 0 for o in offs) and ps[3].grad is None


def test_reference_is_torch_adam_in_float64():
    """the float64 recurrence against torch.optim.Adam on float64 tensors, hyperparameters and resume of A4 / A4r included"""
    for name in ("A4", "A4r"):
        case = R.adam_case(name)
        ref = [x.astype(np.float64) for x in (case.p0, case.m0, case.v0)]
        impl = TorchAdam(case, torch.float64)
        for k in range(case.steps):
            t = case.first_step + k
            R.adam64(*ref, case.grad(k), case.hyper(k), t)
            impl.step(case.grad(k), case.hyper(k), t)
        st = impl.opt.state[impl.p]
        for got, want in zip((impl.p.detach(), st["exp_avg"], st["exp_avg_sq"]), ref):
            assert float(np.abs(got.numpy() - want).max()) <= 1e-13 * max(1.0, float(np.abs(want).max())), name


# ------------------------------------------------------------------------------------------ Adam with the stand-in
class TorchAdam:
    """torch.optim.Adam on the CPU: an operation order of its own (lerp, addcdiv, double scalars)"""

    def __init__(self, case, dtype=torch.float32):
        self.case, self.dtype = case, dtype
        self.p = torch.from_numpy(case.p0.copy()).to(dtype).requires_grad_(True)
        self.opt = None

    def step(self, g, hp, t):
        lr, b1, b2, eps = hp
        if self.opt is None:
            self.opt = torch.optim.Adam([self.p], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
            self.opt.state[self.p] = dict(step=torch.tensor(float(t - 1)),
                                          exp_avg=torch.from_numpy(self.case.m0.copy()).to(self.dtype),
                                          exp_avg_sq=torch.from_numpy(self.case.v0.copy()).to(self.dtype))
        self.opt.param_groups[0]["lr"] = lr
        self.p.grad = torch.from_numpy(g.copy()).to(self.dtype)
        self.opt.step()
        assert int(self.opt.state[self.p]["step"]) == t

    def state(self):
        st = self.opt.state[self.p]
        return [x.detach().numpy() for x in (self.p, st["exp_avg"], st["exp_avg_sq"])]

    def finish(self):
        pass


@pytest.mark.parametrize("name", ["A1", "A2", "A3", "A4", "A4r", "C1", "C2", "C3"])
def test_adam_standin_is_within_every_bound(name):
    R.run_adam(R.adam_case(name), TorchAdam, tag=TAG)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_adam_bound_rejects(mutant):
    """eps inside the root, bc2 without its root, bc1 dropped: each fails the long run A3 in at least one class, by a factor
    of 4 or more; the unmutated formula passes the same call"""
    case = R.adam_case("A3")
    assert R.run_adam(case, R.Numpy32, tag=None) <= 0.25
    ratio = R.run_adam(case, lambda c: R.Numpy32(c, mutant), tag=None, check=False)
    print("%s: worst error / bound = %.3g" % (mutant, ratio))
    assert ratio >= 4.0
    with pytest.raises(AssertionError):
        R.run_adam(case, lambda c: R.Numpy32(c, mutant), tag=None)


def test_a_zero_gradient_that_moves_the_state_is_rejected():
    """the bit-identity of the all-zero class is an assertion of its own: a stand-in that decays p by one part in 2^20 there
    stays far inside 4 x E32 of no class but must fail"""
    case = R.adam_case("A3")
    z = dict(case.classes)["zero"]

    class Leaky(R.Numpy32):
        def step(self, g, hp, t):
            super().step(g, hp, t)
            self.q[0][z] *= np.float32(1 - 2.0 ** -20)
    with pytest.raises(AssertionError, match="not bit-identical"):
        R.run_adam(case, Leaky, tag=None)


# ------------------------------------------------------------------------------------------ the other kernels
class Cpu32:
    """torch / numpy float32 in the place of the kernels of csrc/misc.hip"""

    def __init__(self, mutant=None):
        self.mutant = mutant

    def copy_cols(self, src, dst, rows, ncols, src_ld, src_off, dst_ld, dst_off):
        dst = dst.clone()
        if self.mutant == "copy_first_trip_only":
            rows = min(rows, R.TRIP // ncols)
        dst[:rows * dst_ld].view(rows, dst_ld)[:, dst_off:dst_off + ncols] = \
            src[:rows * src_ld].view(rows, src_ld)[:, src_off:src_off + ncols]
        return dst

    def concat(self, a, b, G):
        a, b = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = torch.cat([a, b], -1)
        (y * G).sum().backward()
        return y.detach(), a.grad, b.grad

    def scale(self, buf, lo, n, a):
        buf = buf.clone()
        buf[lo:lo + (R.TRIP if self.mutant == "scale_first_trip_only" else n)] *= np.float32(a)
        return buf

    def standardize(self, x, mean, std, eps):
        if self.mutant == "eps_dropped":
            return (x - mean.reshape(-1)) / std.reshape(-1).clamp_min(1e-30)
        return (x - mean.reshape(-1)) / (std.reshape(-1) + np.float32(eps))

    def transpose(self, x, buf, lo, B, C, T):
        buf = buf.clone()
        buf[lo:lo + x.numel()] = x.transpose(1, 2).reshape(-1)
        return buf

    def transpose_fn(self, x, G):
        x = x.clone().requires_grad_(True)
        y = x.transpose(1, 2).contiguous()
        (y * G).sum().backward()
        return y.detach(), x.grad

    def colsum(self, X, buf, lo):
        buf = buf.clone()
        rows = X.shape[0] - (1 if self.mutant == "colsum_drops_last_row" else 0)
        buf[lo:lo + X.shape[1]] += X[:rows].sum(0)
        return buf

    def peak(self, w):
        if self.mutant == "peak_signed":
            return w.max(dim=1).values
        return w.abs().max(dim=1).values

    def peak_normalize(self, w):
        return w / self.peak(w)[:, None]


@pytest.mark.parametrize("name", list(R.COPY_CASES))
def test_copy_cols_standin(name):
    R.check_copy_cols(Cpu32(), name, tag=TAG)


@pytest.mark.parametrize("n", R.SCALE_SIZES)
def test_scale_standin(n):
    R.check_scale(Cpu32(), n, tag=TAG)


@pytest.mark.parametrize("name", list(R.STANDARDIZE_CASES))
def test_standardize_standin(name):
    R.check_standardize(Cpu32(), name, tag=TAG)


@pytest.mark.parametrize("shape", R.TRANSPOSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_transpose_standin(shape):
    R.check_transpose(Cpu32(), shape, tag=TAG)


@pytest.mark.parametrize("cols", R.COLSUM_COLS)
@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_colsum_standin(rows, cols):
    R.check_colsum(Cpu32(), rows, cols, tag=TAG)


def test_colsum_bound_is_the_kernels_summation_order():
    """the bound belongs to the kernel's order -- four interleaved row chains per column, their sum, the addition to out -- so a
    float32 numpy evaluation in exactly that order must meet it, at the largest case"""
    rows, cols = 15360, 513

    class KernelOrder(Cpu32):
        def colsum(self, X, buf, lo):
            x = X.numpy()
            s = np.zeros((4, cols), dtype=np.float32)
            for r in range(rows):
                s[r % 4] += x[r]
            buf = buf.clone()
            buf[lo:lo + cols] += torch.from_numpy(((s[0] + s[1]) + s[2]) + s[3])
            return buf
    R.check_colsum(KernelOrder(), rows, cols, tag=TAG)


@pytest.mark.parametrize("L", R.PEAK_LENGTHS)
def test_peak_standin(L):
    R.check_peak(Cpu32(), L, tag=TAG)


@pytest.mark.parametrize("mutant,call", [
    ("copy_first_trip_only", lambda m: R.check_copy_cols(m, "two trips", tag=None)),
    ("scale_first_trip_only", lambda m: R.check_scale(m, R.TRIP + 5, tag=None)),
    ("eps_dropped", lambda m: R.check_standardize(m, "per bin", tag=None)),
    ("colsum_drops_last_row", lambda m: R.check_colsum(m, 5, 65, tag=None)),
    ("peak_signed", lambda m: R.check_peak(m, 1025, tag=None)),
])
def test_kernel_checks_reject(mutant, call):
    """a loop that stops after its first trip, eps left out where std = 0, a dropped row, a peak that ignores the sign"""
    with pytest.raises(AssertionError):
        call(Cpu32(mutant))


def test_hyperparameters_are_rounded_to_float32_first():
    """lr = 1e-3 is not a float32: a reference that kept the double would sit 5e-11 relative away, which the bound need
    not notice -- but bc1 and bc2 from double betas would; the helpers agree with the entry point's arithmetic"""
    lr, b1, b2, eps = R.hyper32(1e-3, 0.9, 0.999, 1e-8)
    assert (lr, b1, b2, eps) == tuple(float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-8))
    bc1, bc2 = R.bias_corrections(b1, b2, 1)
    assert bc1 == 1.0 - float(np.float32(0.9)) and bc2 == 1.0 - float(np.float32(0.999))
    assert bc1 != 1.0 - 0.9 and math.isclose(bc2, 1e-3, rel_tol=1e-4)
