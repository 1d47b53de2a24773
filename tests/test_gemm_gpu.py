"""The dense GEMM entry point ``avvad_gemm_f32`` on the MI355X against tests/gemm_ref.py: every case of its table and sweeps
straight through ctypes (so that relu_a, relu_b, the leading dimensions, the base alignment and the workspace are set
freely), options switched with ``lib_options``.  Exact tier: equality with the float64 product, zero tolerance; rounding
tier: the derived element-wise bound; every float of C outside the M x N output keeps its sentinel bits; every case but the
K-major one runs twice and must be bit-identical run to run.  The workspace is refilled with NaN before every launch: a
fix-up that reads a slab nobody wrote poisons its tile."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import gemm_ref as R
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu
T = torch.from_numpy
_WS = []


def _stream():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ws():
    """the engine's scratch, allocated once for the module and NaN-filled before every launch"""
    from avvad import ops
    if not _WS:
        _WS.append(ops.engine_ws(DEV))
    _WS[0].fill_(float("nan"))
    return _WS[0]


def _desc(d):
    from avvad import _lib as L
    return L.GemmDesc(*(d[k] for k in R.DESC_FIELDS))


def _at(t, off):
    return Ct.c_void_p(t.data_ptr() + 4 * off)


def _launch(bufs, d, A, B, bias, C):
    from avvad import _lib as L
    assert (A.data_ptr() + 4 * bufs.a0) % 16 == 4 * bufs.case["offa"] and (B.data_ptr() + 4 * bufs.b0) % 16 == 4 * bufs.case["offb"]
    ws = _ws() if bufs.ws else None
    dd = _desc(d)
    return L.lib().avvad_gemm_f32(_at(A, bufs.a0), _at(B, bufs.b0), L.ptr(bias), _at(C, bufs.c0), Ct.byref(dd), L.ptr(ws),
                                  0 if ws is None else ws.numel() * 4, _stream())


def hip_impl(bufs, d):
    """the HIP path on the prepared buffers; two runs on fresh copies of C, bit-identical over the whole buffer (guards and
    padding included) unless the K-major cells' float atomics are on"""
    A, B = T(bufs.A_buf).to(DEV), T(bufs.B_buf).to(DEV)
    bias = None if bufs.bias is None else T(bufs.bias).to(DEV)
    outs = []
    for _ in range(2):
        C = T(bufs.C_buf).to(DEV)
        rc = _launch(bufs, d, A, B, bias, C)
        assert rc == 0, "%s: avvad_gemm_f32 returned %d" % (bufs.name, rc)
        outs.append(C)
    torch.cuda.synchronize()
    if not bufs.case["opts"].get("kmajor"):
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), bufs.name + ": two runs differ"
    for what, dev, host in (("A", A, bufs.A_buf), ("B", B, bufs.B_buf), ("bias", bias, bufs.bias)):      # guards included
        assert dev is None or torch.equal(dev.view(torch.int32), T(host).to(DEV).view(torch.int32)), "%s: %s was written" % (bufs.name, what)
    bufs.C_buf[:] = outs[0].cpu().numpy()


def _run(name, lib_options):
    for k, v in R.CASES[name]["opts"].items():
        lib_options(k, v)
    return R.check_gemm(hip_impl, name, tag="gpu")


@pytest.mark.parametrize("name", R.TABLE)
def test_schedule_table(name, lib_options):
    """every plan branch: both tiles; data-parallel rounds only, a partially filled last round, a pool with and without full
    rounds and with G capped; dense and sparse pools on both fix-up kernels and their second loop iterations"""
    _run(name, lib_options)


@pytest.mark.parametrize("name", R.FORMS)
def test_operand_forms_and_leading_dimensions(name, lib_options):
    """the four transpositions x the vector and the scalar form of each operand (by shape, by ld % 4, by a base 4 bytes off
    16), ld tight and padded by 4 and 5: NaN padding never enters a product, C's padding keeps its bits"""
    _run(name, lib_options)


@pytest.mark.parametrize("name", R.EPILOGUES)
def test_epilogues(name, lib_options):
    _run(name, lib_options)


@pytest.mark.parametrize("name", R.RELU)
def test_fused_relu(name, lib_options):
    _run(name, lib_options)


@pytest.mark.parametrize("name", [s[0] for s in R.OPTION_SWEEP] + R.OPTION_BASES)
def test_engine_options(name, lib_options):
    _run(name, lib_options)


@pytest.mark.parametrize("name", R.ROUNDING)
def test_rounding_tier(name, lib_options):
    ratio = _run(name, lib_options)
    assert ratio > 0, "a float32 product of N(0, 1) operands that equals the float64 one everywhere is not what was asked for"


def test_log_the_worst_rounding_ratio():
    R.log_worst("gpu")


def test_exact_tier_is_bit_identical_across_worker_counts(lib_options):
    """300 x 333 x 513 on 4, 3 and 1 CUs (G = 8, 6, 2) and on the whole chip: different splits of the same exact sums"""
    outs = []
    for cus in (4, 3, 1, 0):
        lib_options("max_cus", cus)
        bufs = R.prepare("300x333x513-c3")
        hip_impl(bufs, bufs.d)
        outs.append(bufs.C_buf.copy())
    assert all(np.array_equal(outs[0].view(np.uint32), o.view(np.uint32)) for o in outs[1:])


def test_refusals_leave_c_untouched():
    """split_k > 1 without accumulate, bias with split_k > 1, M, N or K <= 0, NULL for A, B, C or the descriptor, a workspace
    4 bytes off its alignment: AVVAD_EINVAL, and not one bit of C changes"""
    from avvad import _lib as L
    name = "form-tA0-tB0-pad4"
    bufs = R.prepare(name)
    A, B, C = T(bufs.A_buf).to(DEV), T(bufs.B_buf).to(DEV), T(bufs.C_buf).to(DEV)
    bias = T(np.ones(bufs.d["N"], dtype=np.float32)).to(DEV)
    before = C.clone()
    ws = _ws()
    lib = L.lib()

    def call(a=A, b=B, c=C, bias=None, desc=True, ws_off=0, **change):
        dd = _desc(dict(bufs.d, **change))
        return lib.avvad_gemm_f32(None if a is None else _at(a, bufs.a0), None if b is None else _at(b, bufs.b0), L.ptr(bias),
                                  None if c is None else _at(c, bufs.c0), Ct.byref(dd) if desc else None,
                                  Ct.c_void_p(ws.data_ptr() + ws_off), ws.numel() * 4 - 16, _stream())
    assert call(split_k=4, accumulate=0) == R.EINVAL
    assert call(split_k=4, accumulate=1, bias=bias) == R.EINVAL
    for dim in ("M", "N", "K"):
        assert call(**{dim: 0}) == R.EINVAL and call(**{dim: -3}) == R.EINVAL
    assert call(a=None) == R.EINVAL and call(b=None) == R.EINVAL and call(c=None) == R.EINVAL and call(desc=False) == R.EINVAL
    assert call(ws_off=4) == R.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(C.view(torch.int32), before.view(torch.int32))
    assert call(ws_off=0) == 0                    # (the same call goes through once nothing is wrong with it)
    torch.cuda.synchronize()
    assert not torch.equal(C.view(torch.int32), before.view(torch.int32))


@pytest.mark.parametrize("M,form", [((1 << 20) - 1, "RowVec4"), (1 << 20, "RowPlain")])
def test_the_2gib_switch_of_rowvec4(M, form):
    """N = 64, K = 32, lda = 512: at M = 2^20 - 1 the last 16-byte fetch of RowVec4 ends 1952 bytes below 2^31; at M = 2^20
    (M lda = 2^29) the entry point switches to RowPlain and 64-bit addresses.  Exact tier; the 480 padding columns of every row
    of A are NaN.  The reference is the float64 product of A[:, :K] copied to the host (128 MB), over ALL rows."""
    from avvad import _lib as L
    N, K, lda = 64, 32, 512
    d = dict(M=M, N=N, K=K, lda=lda, ldb=N, ldc=N, transA=0, transB=0, accumulate=0, split_k=1, relu_a=0, relu_b=0)
    assert R.gemm_plan(d)["a_form"] == form and ((M - 1) * lda + K) * 4 < 1 << 31
    g = torch.Generator(device=DEV).manual_seed(M % 1000)
    A = torch.full((R.GUARD + M * lda + R.GUARD,), float("nan"), device=DEV)
    mag = torch.randint(0, 9, (M, K), device=DEV, generator=g).float()
    A[R.GUARD:R.GUARD + M * lda].view(M, lda)[:, :K] = torch.where(torch.rand(M, K, device=DEV, generator=g) < 1 / 3, -mag, mag)
    Bh = R._draw(np.random.default_rng(M), "exact", K, N)
    B = T(R._padded(Bh, N, 0, np.nan)).to(DEV)
    C = torch.full((R.GUARD + M * N + R.GUARD,), -0.0, device=DEV)
    ws = _ws()
    rc = L.lib().avvad_gemm_f32(_at(A, R.GUARD), _at(B, R.GUARD), None, _at(C, R.GUARD), Ct.byref(_desc(d)), L.ptr(ws),
                                ws.numel() * 4, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    Ah = A[R.GUARD:R.GUARD + M * lda].view(M, lda)[:, :K].cpu()
    ref = (Ah.double() @ T(Bh).double()).float()
    got = C.cpu()
    for guard in (got[:R.GUARD], got[R.GUARD + M * N:]):
        assert bool((guard.view(torch.int32) == -(1 << 31)).all()), "the guard around C was written"
    got = got[R.GUARD:R.GUARD + M * N].view(M, N)
    wrong = (got != ref).nonzero()
    assert wrong.numel() == 0, "%d elements differ, the first at %s, rows %d .. %d" % (
        len(wrong), wrong[0].tolist(), int(wrong[:, 0].min()), int(wrong[:, 0].max()))
