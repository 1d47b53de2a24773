"""The single-convolution entry points ``avvad_conv2d_{pack_weights,fwd,dgrad,wgrad}`` and their ``_bf16`` twins on the MI355X
against tests/conv_ref.py: every case of its lists straight through ctypes, options switched with ``lib_options``.  Exact
tier: equality with the float64 reference, zero tolerance; rounding tier: the derived element-wise bound.  Every operand sits
between NaN guards, every output between -0.0 guards that must keep their bits; the engine scratch is refilled with NaN
before every launch; every product runs twice and must be bit-identical run to run; the inputs must be unchanged; the weight
packs come from the pack entry points and are compared bit for bit with the layouts conv_ref restates.  A refused call must
return AVVAD_EINVAL and leave every bit of its output buffer."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import conv_ref as R
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


def _at(t):
    """the logical origin of a guarded device buffer"""
    return Ct.c_void_p(t.data_ptr() + R.GUARD * t.element_size())


def _desc(d):
    from avvad import _lib as L
    return L.ConvDesc(*(d[k] for k in R.DESC_FIELDS))


def _same_bits(a, b):
    it = torch.int32 if a.element_size() == 4 else torch.int16
    return torch.equal(a.view(it), b.view(it))


def _device_side(bufs):
    """uploads the operands of a case once (bf16 on the _bf16 path: the values are exact in it) and packs the weights on the
    device: the packs must equal conv_ref's restated layouts bit for bit, inside untouched -0.0 guards"""
    from avvad import _lib as L
    lib, g, b16 = L.lib(), bufs.g, bufs.path == "b16"
    dt = torch.bfloat16 if b16 else torch.float32
    dev = bufs.dev = {"x": T(bufs.x_buf).to(DEV).to(dt), "dy": T(bufs.dy_buf).to(DEV).to(dt)}
    w = T(bufs.w_buf).to(DEV)
    n = g.KS * g.KS * g.C * g.Co
    wf, wd = (torch.full((R.GUARD + n + R.GUARD,), -0.0, device=DEV, dtype=dt) for _ in range(2))
    dd = _desc(bufs.d)
    pack = lib.avvad_conv2d_pack_weights_bf16 if b16 else lib.avvad_conv2d_pack_weights
    rc = pack(_at(w), _at(wf), _at(wd), Ct.byref(dd), _stream())
    torch.cuda.synchronize()
    if b16 and (g.C % 64 or g.Co % 64):
        assert rc == R.EINVAL and _same_bits(wf, torch.full_like(wf, -0.0)) and _same_bits(wd, torch.full_like(wd, -0.0))
    else:
        assert rc == 0, "%s: the pack entry point returned %d" % (bufs.name, rc)
        wl = R.view(bufs, "wf_buf"), R.view(bufs, "wd_buf")
        if b16:
            flat = bufs.w_buf[R.GUARD:R.GUARD + n]
            i_f, i_d = R.pack_bf16_index(g.Co, g.C, g.KS)
            wl = np.empty(n, np.float32), np.empty(n, np.float32)
            wl[0][i_f], wl[1][i_d] = flat, flat
        for got, want, what in ((wf, wl[0], "wf"), (wd, wl[1], "wd")):
            exp = torch.full_like(got, -0.0)
            exp[R.GUARD:R.GUARD + n] = T(np.ascontiguousarray(want).reshape(-1)).to(DEV).to(dt)
            assert _same_bits(got, exp), "%s: the %s pack differs from the restated layout, or its guards were written" % (bufs.name, what)
    assert _same_bits(w, T(bufs.w_buf).to(DEV)), bufs.name + ": the pack entry point wrote w"
    for t in (wf, wd):                                   # the packs as operands: NaN guards
        t[:R.GUARD] = float("nan")
        t[R.GUARD + n:] = float("nan")
    dev["wf"], dev["wd"] = wf, wd
    dev["pristine"] = {k: v.clone() for k, v in dev.items()}


def hip_impl(bufs, direction):
    """the HIP path on the prepared buffers; two runs on fresh copies of the output, bit-identical over the whole buffer"""
    from avvad import _lib as L
    lib, b16 = L.lib(), bufs.path == "b16"
    if not hasattr(bufs, "dev"):
        _device_side(bufs)
    dev, dd = bufs.dev, _desc(bufs.d)
    host = getattr(bufs, R.OUT_BUF[direction])
    sfx = "_bf16" if b16 else ""
    outs, rcs = [], []
    for _ in range(2):
        out = T(host).to(DEV)
        ws = _ws() if bufs.ws else None
        wsa = (L.ptr(ws), 0 if ws is None else ws.numel() * 4, _stream())
        if direction == "fwd":
            rc = getattr(lib, "avvad_conv2d_fwd" + sfx)(_at(dev["x"]), _at(dev["wf"]), _at(out), Ct.byref(dd), *wsa)
        elif direction == "dgrad":
            rc = getattr(lib, "avvad_conv2d_dgrad" + sfx)(_at(dev["dy"]), _at(dev["wd"]), _at(out), Ct.byref(dd), bufs.acc, *wsa)
        else:
            rc = getattr(lib, "avvad_conv2d_wgrad" + sfx)(_at(dev["x"]), _at(dev["dy"]), _at(out), Ct.byref(dd), *wsa)
        outs.append(out)
        rcs.append(rc)
    torch.cuda.synchronize()
    assert rcs[0] == rcs[1] and _same_bits(outs[0], outs[1]), "%s %s: two runs differ" % (bufs.name, direction)
    for k, v in dev["pristine"].items():                 # guards included
        assert _same_bits(dev[k], v), "%s %s: operand %s was written" % (bufs.name, direction, k)
    host[:] = outs[0].cpu().numpy()
    return rcs[0]


def _run(name, lib_options):
    for k, v in R.CASES[name]["opts"].items():
        lib_options(k, v)
    return R.check_conv(hip_impl, name, tag="gpu")


@pytest.mark.parametrize("name", R.SWEEP)
def test_engine_kernel_stride_pad_sweep(name, lib_options):
    """KS 1 .. 5 x stride 1, 2 x pad {0, KS // 2, KS - 1} on a 7 x 5 image: the im2col engine's tap masks, the parity classes
    of every even and odd kernel, and the KS = 5 / stride 2 data gradient refused with dx untouched"""
    _run(name, lib_options)


@pytest.mark.parametrize("name", R.ENGINE)
def test_engine_tiles_schedules_and_options(name, lib_options):
    """H or W of 1, KS > H, Co in {4, 36, 64, 68, 160}, the tall tile and no_tall, whole tiles and stream-K with split tiles,
    both fix-up kernels, no_streamk, no_buf, capped grids, accumulate 0 and 1, option bf16 = 1"""
    _run(name, lib_options)


@pytest.mark.parametrize("name", R.PARITY)
def test_stride2_data_gradient_by_parity_classes(name, lib_options):
    _run(name, lib_options)


@pytest.mark.parametrize("name", R.STEM)
def test_one_channel_input(name, lib_options):
    """the LDS-resident stem kernels, their fall-backs (odd Wo, Wo > 34, a frame just over the LDS budget, no workspace,
    no_stem_kernel), Co 32 and 128 and 3x3 / 5x5 kernels through the engine's scalar gathers; the data gradient is refused"""
    _run(name, lib_options)


@pytest.mark.parametrize("name", R.CONV64)
def test_conv64_kernels(name, lib_options):
    _run(name, lib_options)


@pytest.mark.parametrize("name", R.CLS)
def test_position_classes_and_taps(name, lib_options):
    """grids 2x2 .. 5x4, 128 / 129 / 257 images, ragged column tiles, stride 2 at every parity of H and W, the stride-2 data
    gradient as one class product and as four launches, no_cls, the tile cap from both sides, Ho = 1, 127 images"""
    _run(name, lib_options)


@pytest.mark.parametrize("name", R.B16)
def test_bf16_data_path(name, lib_options):
    _run(name, lib_options)


@pytest.mark.parametrize("name", R.REFUSALS)
def test_refusals_by_shape(name, lib_options):
    _run(name, lib_options)


@pytest.mark.parametrize("name", R.ROUNDING)
def test_rounding_tier(name, lib_options):
    ratio = _run(name, lib_options)
    assert ratio > 0, "a float32 convolution of N(0, 1) operands that equals the float64 one everywhere is not what was asked for"


def test_log_the_worst_rounding_ratio():
    R.log_worst("gpu")


def test_refusals_by_descriptor_and_pointers():
    """what conv_geom refuses (non-positive dimensions, a negative pad, stride 3, a kernel that fits nowhere -- (H + 2 pad - KS)
    / 2 = -1 / 2 rounds to 0 in C), NULL operands and a workspace 4 bytes off its alignment: AVVAD_EINVAL from every entry point,
    and not one bit of any output changes"""
    from avvad import _lib as L
    lib = L.lib()
    ok = dict(N=2, H=5, W=5, C=64, Co=64, KS=3, stride=1, pad=1)
    n = 4096 * 16
    src = torch.ones(n, device=DEV)
    src16 = torch.ones(n, device=DEV, dtype=torch.bfloat16)
    out = torch.full((n,), -0.0, device=DEV)
    out16 = torch.full((n,), -0.0, device=DEV, dtype=torch.bfloat16)
    before, before16 = out.clone(), out16.clone()
    ws = _ws()
    st = _stream()

    def calls(d, a=src, a16=src16, o=out, o16=out16, ws_off=0):
        dd = Ct.byref(_desc(d)) if d is not None else None
        wsa = (Ct.c_void_p(ws.data_ptr() + ws_off), ws.numel() * 4 - 16, st)
        p = L.ptr
        packs = [] if ws_off else [lib.avvad_conv2d_pack_weights(p(a), p(o), p(o), dd, st),
                                   lib.avvad_conv2d_pack_weights_bf16(p(a), p(o16), p(o16), dd, st)]      # (they take no workspace)
        return packs + [lib.avvad_conv2d_fwd(p(a), p(a), p(o), dd, *wsa), lib.avvad_conv2d_fwd_bf16(p(a16), p(a16), p(o), dd, *wsa),
                lib.avvad_conv2d_dgrad(p(a), p(a), p(o), dd, 0, *wsa), lib.avvad_conv2d_dgrad_bf16(p(a16), p(a16), p(o), dd, 1, *wsa),
                lib.avvad_conv2d_wgrad(p(a), p(a), p(o), dd, *wsa), lib.avvad_conv2d_wgrad_bf16(p(a16), p(a16), p(o), dd, *wsa)]
    bad = [dict(ok, **{k: v}) for k in ("N", "H", "W", "C", "Co", "KS", "stride") for v in (0, -2)]
    bad += [dict(ok, pad=-1), dict(ok, stride=3), dict(ok, H=2, pad=0, stride=2), dict(ok, W=1, KS=4, stride=2), None]
    for d in bad:
        assert d is None or R.geom(d) is None
        assert calls(d) == [R.EINVAL] * 8, d
    assert calls(ok, a=None, a16=None) == [R.EINVAL] * 8 and calls(ok, o=None, o16=None) == [R.EINVAL] * 8
    assert calls(ok, ws_off=4) == [R.EINVAL] * 6
    torch.cuda.synchronize()
    assert _same_bits(out, before) and _same_bits(out16, before16)
    assert calls(ok)[2] == 0                               # (the same call goes through once nothing is wrong with it)
    torch.cuda.synchronize()
    assert not _same_bits(out, before)


def test_exact_tier_is_bit_identical_across_worker_counts(lib_options):
    """the stream-K case on 2, 3, 8 CUs and on the whole chip: different splits of the same exact sums"""
    outs = []
    for cus in (2, 3, 8, 0):
        lib_options("max_cus", cus)
        bufs = R.prepare("sk")
        for direction in R.DIRECTIONS:
            assert hip_impl(bufs, direction) == 0
        outs.append(np.concatenate([bufs.y_buf, bufs.dx_buf, bufs.dw_buf]).view(np.uint32))
    assert all(np.array_equal(outs[0], o) for o in outs[1:])
