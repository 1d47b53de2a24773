"""The caller-owned buffer contract of include/avvad.h, one case per entry-point family (tests/abi_guard.py):

  (a) what a workspace or an output holds on entry never reaches a result -- every case runs with zero-, NaN- and
      1e30-filled buffers and must return the same bits (``torch.equal``);
  (b) nothing outside the workspace is written -- 65536 guard floats on either side keep their pattern;
  (c) a workspace one float below the queried size is refused (AVVAD_EWORKSPACE) with every buffer still poisoned -- a
      run of its own for EVERY entry point a case goes through (a refused call raises, so one run reaches one entry
      point), the backward entry points included: those get the forward's workspace declared 4 bytes shorter;
  and the pointer classes: entry points that pick a vector or a scalar form from a pointer's alignment are run in both
  forms, a workspace 4 bytes off its 16-byte alignment is refused (AVVAD_EINVAL) before anything is launched.

Each case builds its inputs once and returns the dict of its results (outputs and every gradient).  The workspace is
poisoned when it is allocated, i.e. BEFORE THE FORWARD ONLY: the backward entry points read what the forward left in it
(``ctx``), and the contract says so.  The NaN run is then compared with the reference of the op's existing parity test
(oracle, golden file, float64 numpy or a ``*_ref.py``), at that test's tolerance and on its inputs: the helpers are
imported from those tests, no bound is derived here.

No result is compared with a bound across the fills: the count sketch, once the library's one unordered sum (LDS
atomics), adds its buckets in a fixed order (csrc/mcb.hip ``sketch_row``), and so does the fusion's norm.
"""
import ctypes as Ct
import os
import random

import numpy as np
import pytest
import torch

import stategen
from abi_guard import Guard, expect_backward_refused, expect_refused, guarded, run_contract, run_direct
from conftest import load_golden, wn_cfg_from
from test_gpu_parity import DEV, OUT, T, _grad_bound, _relu_flips, _report, _report_grad, _video_state

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _ops():
    from avvad import ops
    return ops


def _contract(monkeypatch, case, **kw):
    os.makedirs(OUT, exist_ok=True)
    return run_contract(monkeypatch, _ops(), case, **kw)


def _backward_refused(monkeypatch, entry, forward, backward):
    """The backward entry point ``entry`` refuses the forward's workspace one float short (AVVAD_EWORKSPACE) and 4 bytes off
    its alignment (AVVAD_EINVAL), both before it launches anything."""
    expect_backward_refused(monkeypatch, _ops(), entry, forward, backward)
    expect_backward_refused(monkeypatch, _ops(), entry, forward, backward, match="AVVAD_EINVAL", misaligned=True)


def _out(*shape):
    """An output buffer the CASE owns, allocated the way ``ops`` allocates its own: poisoned and registered while a guard
    is installed."""
    return _ops().torch.empty(*shape, dtype=torch.float32, device=DEV)


def _stream():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rehome(t, off=1):
    """The same values, contiguous, ``off`` floats behind a fresh block's 256-byte boundary: ``buf[off:off + n].view(shape)``."""
    buf = torch.empty(t.numel() + off + 3, dtype=t.dtype, device=t.device)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
    return v


# =========================================================================================== engine / GEMM
def _gemm_operands(M, N, K, tA, tB):
    """test_gemm_variants' operands and float64 product"""
    rng = np.random.RandomState(M + N + K)
    A = rng.normal(size=(K, M) if tA else (M, K)).astype(np.float32)
    B = rng.normal(size=(N, K) if tB else (K, N)).astype(np.float32)
    bias = rng.normal(size=(N,)).astype(np.float32)
    ref = (A.T if tA else A).astype(np.float64) @ (B.T if tB else B).astype(np.float64)
    return A, B, bias, ref


def test_gemm_ragged_with_bias_and_split_k_accumulate(monkeypatch):
    """(100, 70, 513) tB + bias: ragged tiles, rows of 513 floats (scalar loads); then accumulate=True, split_k=4 onto a
    given C.  The engine's scratch is optional (see the slab test for what a short one does)."""
    ops = _ops()
    M, N, K, tA, tB = 100, 70, 513, 0, 1
    A, B, bias, ref = _gemm_operands(M, N, K, tA, tB)
    a, b, bs = T(A).to(DEV), T(B).to(DEV), T(bias).to(DEV)
    c0 = torch.randn(M, N, device=DEV)

    def case():
        c = _out(M, N)
        ops.gemm(a, b, c, M, N, K, A.shape[1], B.shape[1], N, bool(tA), bool(tB), bias=bs)
        c1 = c0.clone()
        ops.gemm(a, b, c1, M, N, K, A.shape[1], B.shape[1], N, bool(tA), bool(tB), accumulate=True, split_k=4)
        return {"c": c, "c_acc": c1}
    got = _contract(monkeypatch, case, short=None)
    _report("contract: gemm 100x70x513 tB +bias", got["c"], ref + bias, 1e-5 * np.sqrt(K) * 4)
    _report("contract: gemm 100x70x513 split-k accumulate", got["c_acc"], ref + c0.cpu().numpy(), 1e-5 * np.sqrt(K) * 4)


@pytest.mark.parametrize("M,N,K", [(700, 4096, 40), (64, 1024, 4096)])
def test_gemm_stream_k_slab_and_the_short_slab_exception(M, N, K, monkeypatch):
    """test_engine_streamk_fixup_equals_whole_tile's two small shapes: K so short that most workers of the stream-K round
    get an EMPTY share of the slab, and fewer tiles than workers.  Reference, as there: the whole-tile schedule (ws = NULL).
    The documented exception to (c): below avvad_engine_workspace() bytes avvad_gemm_f32 takes the whole-tile schedule --
    ``need - 4`` bytes return OK, the bits of ws = NULL, and leave the buffer alone."""
    from avvad import _lib as L
    ops = _ops()
    rng = np.random.RandomState(M % 1000 + K)
    A = T(rng.normal(size=(M, K)).astype(np.float32)).to(DEV)
    B = T(rng.normal(size=(K, N)).astype(np.float32)).to(DEV)
    bias = T(rng.normal(size=(N,)).astype(np.float32)).to(DEV)
    lib = L.lib()
    d = L.GemmDesc(M, N, K, K, N, N, 0, 0, 0, 1, 0, 0)
    whole = torch.full((M, N), 7.0, device=DEV)
    L.check(lib.avvad_gemm_f32(L.ptr(A), L.ptr(B), L.ptr(bias), L.ptr(whole), Ct.byref(d), None, 0, _stream()), "gemm, no scratch")

    def case():
        c = _out(M, N)
        ops.gemm(A, B, c, M, N, K, K, N, N, bias=bias)
        acc = torch.full((M, N), 0.5, device=DEV)
        ops.gemm(A, B, acc, M, N, K, K, N, N, accumulate=True, split_k=4)
        return {"c": c, "acc": acc}
    got = _contract(monkeypatch, case, short=None)
    _report("contract: engine %dx%dx%d stream-K vs whole-tile" % (M, N, K), got["c"], whole, 2e-5 * np.sqrt(K), 1e-5)
    _report("contract: engine %dx%dx%d accumulate" % (M, N, K), got["acc"], whole - bias + 0.5, 2e-5 * np.sqrt(K), 1e-5)
    need = lib.avvad_engine_workspace()
    g = Guard(NAN, short=True)
    ws = g.workspace(need // 4, DEV)
    assert ws.numel() * 4 == need - 4
    c = g.new_output(M, N, device=DEV)
    assert lib.avvad_gemm_f32(L.ptr(A), L.ptr(B), L.ptr(bias), L.ptr(c), Ct.byref(d), L.ptr(ws), ws.numel() * 4, _stream()) == 0
    assert torch.equal(c, whole)
    g.outputs.clear()                      # (c was written, as it must be; the workspace and its guards were not)
    g.assert_untouched()


def test_linear_fn_forward_and_backward(monkeypatch):
    """LinearFn at 37 x 130 x 96 (test_gemm_variants' ragged NN shape): y, dx, dW, db against float64."""
    ops = _ops()
    rng = np.random.RandomState(37 + 130 + 96)
    X, W, Bv, G = (rng.normal(size=s).astype(np.float32) for s in ((37, 96), (130, 96), (130,), (37, 130)))
    x, w, b, gd = (T(v).to(DEV) for v in (X, W, Bv, G))

    def case():
        xg, wg, bg = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = ops.LinearFn.apply(xg, wg, bg)
        (y * gd).sum().backward()
        return {"y": y, "dx": xg.grad, "dw": wg.grad, "db": bg.grad}
    got = _contract(monkeypatch, case, short=None)
    X64, W64, G64 = X.astype(np.float64), W.astype(np.float64), G.astype(np.float64)
    tol = lambda k: 1e-5 * np.sqrt(k) * 4               # test_gemm_variants, K the contraction length
    _report("contract: LinearFn y", got["y"], X64 @ W64.T + Bv, tol(96))
    _report("contract: LinearFn dx", got["dx"], G64 @ W64, tol(130))
    _report("contract: LinearFn dW", got["dw"], G64.T @ X64, tol(37))
    _report("contract: LinearFn db", got["db"], G64.sum(0), tol(37))


# =========================================================================================== LSTM
@pytest.mark.parametrize("B,H,Tn,per_step,layers", [(16, 256, 5, 0, 1), (16, 256, 5, 1, 1), (128, 128, 3, 0, 1), (3, 32, 4, 0, 1),
                                                     (3, 32, 4, 0, 2)])
def test_lstm_layers(B, H, Tn, per_step, layers, monkeypatch, lib_options):
    """test_lstm_fused_step_sequence_groups' set-up (In = 40, oracle time loop): the persistent launch (flags and hand-off
    copies in the slab), the same shape with per-step kernels, lstm_step_fwd_mfma<4>, the GEMM + gates path with the
    unfused backward, and a two-layer stack.  Ragged lengths with one full row and one of length 1: the padded steps of y
    and of every saved buffer are never written by a step kernel."""
    import torch.nn as nn
    from oracle import head
    ops = _ops()
    if per_step:
        lib_options("lstm_no_persistent", 1)
    torch.manual_seed(B + H + layers)
    In = 40
    lstm = nn.LSTM(In, H, layers)
    x = torch.randn(B, Tn, In)
    lens = [int(v) for v in torch.randint(1, Tn + 1, (B,))]
    lens[0], lens[1] = Tn, 1
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in lstm.state_dict().items()}
    xr = x.clone().requires_grad_(True)
    ref = head.lstm_stack(xr, lens, sd, "", layers)
    Gd = torch.randn(B, Tn, H)
    (ref * Gd).sum().backward()
    lstm = lstm.to(DEV)
    xd, gd = x.to(DEV), Gd.to(DEV)

    def case():
        for p in lstm.parameters():
            p.grad = None
        xg = xd.clone().requires_grad_(True)
        y = ops.lstm_stack(xg, lens, lstm)
        (y * gd).sum().backward()
        return dict({"y": y, "dx": xg.grad}, **{k: p.grad for k, p in lstm.named_parameters()})
    got = _contract(monkeypatch, case)
    _backward_refused(monkeypatch, "avvad_lstm_layer_bwd", lambda: ops.lstm_stack(xd.clone().requires_grad_(True), lens, lstm),
                      lambda y: (y * gd).sum().backward())
    tag = "contract: lstm B=%d H=%d T=%d%s x%d" % (B, H, Tn, " per-step" if per_step else "", layers)
    _report(tag + " forward", got["y"], ref, 1e-4)
    _report_grad(tag + " d/dx", got["dx"], xr.grad)
    for k in sd:
        _report_grad(tag + " d/d" + k, got[k], sd[k].grad)


# =========================================================================================== WaveNet encoder
@pytest.mark.parametrize("name", ["wn_tiny", "wn_fw3_qc2", "wn_w0_t16"])
def test_wavenet_goldens(name, monkeypatch):
    """test_wavenet_golden (default kernel forms): forward, d/dx and every parameter gradient against the reference's own."""
    from packages.models.wavenet_autoencoder import wavenet_autoencoder
    g = load_golden(name)
    m = wavenet_autoencoder(**wn_cfg_from(g))
    m.load_state_dict({k[2:]: T(v) for k, v in g.items() if k.startswith("p.")})
    m = m.to(DEV)
    xd, Gd = T(g["x"]).to(DEV), T(g["G"]).to(DEV)

    def case():
        for p in m.parameters():
            p.grad = None
        x = xd.clone().requires_grad_(True)
        y = m(x)
        (y * Gd).sum().backward()
        return dict({"y": y, "dx": x.grad}, **{"g." + k: p.grad for k, p in m.named_parameters()})
    got = _contract(monkeypatch, case)
    _backward_refused(monkeypatch, "avvad_wavenet_bwd", lambda: m(xd.clone().requires_grad_(True)), lambda y: (y * Gd).sum().backward())
    _report("contract: " + name + " forward", got["y"], g["y"], 1e-4)
    _report_grad("contract: " + name + " d/dx", got["dx"], g["dx"], rel_bound=2e-3)
    for k, _ in m.named_parameters():
        _report_grad("contract: " + name + " d/d" + k, got["g." + k], g["g." + k], rel_bound=2e-3)


# =========================================================================================== trunk
@pytest.mark.parametrize("training,streamk", [(True, False), (False, False), (True, True)])
def test_trunk_forward_and_backward(training, streamk, monkeypatch, lib_options):
    """test_trunk_backward_vs_oracle on the video_h16 golden model: features, the running statistics (train mode) and the
    gradient of every trunk parameter; whole-tile schedule, and once the production stream-K schedule.  The ReLU-flip
    count that opens the gradient bound is taken in the NaN run, like everything that is compared with the oracle."""
    from avvad import nn as avnn
    from oracle import resnet18
    from packages.models.Video_Net import DeepVAD_video
    os.makedirs(OUT, exist_ok=True)
    lib_options("no_streamk", 0 if streamk else 1)
    sd0 = _video_state()
    N = 6
    x = stategen.rand(21, N, 67, 67)
    G = stategen.rand(22, N, 512)
    sd = {k: (v.clone().requires_grad_(True) if v.dtype == torch.float32 and "running" not in k else v.clone())
          for k, v in sd0.items() if k.startswith("features.")}
    ref, inter = resnet18.trunk_forward(sd, x[:, None].repeat(1, 3, 1, 1), training, return_intermediates=True)
    (ref * G).sum().backward()
    m = DeepVAD_video(2, 16, 1)
    m.load_state_dict(sd0)
    m = m.to(DEV).train(training)
    xd, gd = x.to(DEV), G.to(DEV)
    flips = []

    def case():
        m.load_state_dict(sd0)                    # (train mode moves the running statistics: every run starts from the same)
        for p in m.features.parameters():
            p.grad = None
        f = avnn.trunk_forward(m.features, xd, training)
        flips.append(_relu_flips(f, inter)[0])
        (f * gd).sum().backward()
        out = {"f": f}
        out.update({"g." + k: p.grad for k, p in m.features.named_parameters()})
        out.update({"b." + k: b.clone() for k, b in m.features.named_buffers() if "running" in k})
        return out
    got = _contract(monkeypatch, case)
    _backward_refused(monkeypatch, "avvad_trunk_bwd", lambda: avnn.trunk_forward(m.features, xd, training), lambda f: (f * gd).sum().backward())
    tag = "contract: trunk (training=%s, streamk=%s)" % (training, streamk)
    _report(tag + " fwd", got["f"], ref, 1e-4, 1e-5)
    rel = _grad_bound(flips[1], 2e-3 if not training else 5e-3)           # flips[1]: the NaN run's count
    for k, _ in m.features.named_parameters():
        _report_grad(tag + " d/d%s" % k, got["g." + k], sd["features." + k].grad, 2.0, rel)
    if training:                                  # test_video_net_golden_eval_and_train's bound on the running statistics
        for k, _ in m.features.named_buffers():
            if "running" in k:
                _report(tag + " " + k, got["b." + k], sd["features." + k], 1e-5, 1e-5)


# =========================================================================================== stand-alone convolutions
CONV_SHAPES = [(3, 17, 17, 64, 64, 3, 1, 1), (2, 17, 17, 64, 128, 3, 2, 1), (5, 9, 9, 128, 128, 3, 1, 1), (130, 3, 3, 512, 512, 3, 1, 1)]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("N,H,W,C,Co,KS,stride,pad", CONV_SHAPES)
def test_conv2d_entry_points_direct(N, H, W, C, Co, KS, stride, pad, bf16):
    """avvad_conv2d_{fwd,dgrad,wgrad} and their _bf16 twins through the C ABI with a guarded engine scratch and poisoned
    outputs (the weight packs included), against F.conv2d + autograd with the operands, seeds and bounds of
    test_conv2d_fwd_dgrad_wgrad, test_conv2d_position_classes_skip_the_zero_padding (130 images on a 3x3 grid: the
    position-class schedule) and test_bf16_data_path_convolutions.  Then the documented exception to (c): ``need - 4``
    bytes of scratch return OK with the bits of ws = NULL and leave the buffer alone.  A scratch pointer 4 bytes off
    its 16-byte alignment is refused (AVVAD_EINVAL) by each of the three with nothing launched."""
    import torch.nn.functional as F
    from avvad import _lib as L
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    cls = N == 130
    rng = np.random.RandomState(N * H + C + 7 if bf16 else (N + H * 7 + C if cls else N * H + C))
    r16 = (lambda t: t.bfloat16().float()) if bf16 else (lambda t: t)
    x = r16(T(rng.normal(size=(N, C, H, W)).astype(np.float32))).requires_grad_(True)
    w = r16(T((rng.normal(size=(Co, C, KS, KS)) / np.sqrt(C * KS * KS)).astype(np.float32))).requires_grad_(True)
    y = F.conv2d(x, w, None, stride, pad)
    gy = r16(T(rng.normal(size=tuple(y.shape)).astype(np.float32)))
    y.backward(gy)
    wref = w.grad.permute(2, 3, 1, 0).reshape(KS * KS * C, Co)
    lib = L.lib()
    d = L.ConvDesc(N, H, W, C, Co, KS, stride, pad)
    dt = torch.bfloat16 if bf16 else torch.float32
    xd = x.detach().permute(0, 2, 3, 1).contiguous().to(DEV).to(dt)
    gyd = gy.permute(0, 2, 3, 1).contiguous().to(DEV).to(dt)
    wdev = w.detach().to(DEV)
    need = lib.avvad_engine_workspace()
    fwd, dgrad, wgrad, pack = ((lib.avvad_conv2d_fwd_bf16, lib.avvad_conv2d_dgrad_bf16, lib.avvad_conv2d_wgrad_bf16,
                                lib.avvad_conv2d_pack_weights_bf16) if bf16 else
                               (lib.avvad_conv2d_fwd, lib.avvad_conv2d_dgrad, lib.avvad_conv2d_wgrad, lib.avvad_conv2d_pack_weights))
    Ho, Wo = y.shape[2], y.shape[3]

    def run(g, ws, rc=0):
        wsz = 0 if ws is None else ws.numel() * 4
        nw = KS * KS * C * Co
        if bf16:                                  # (bf16 packs are no float32 outputs: poisoned by hand)
            wf, wdg = (torch.full((nw,), g.fill, dtype=dt, device=DEV) for _ in range(2))
        else:
            wf, wdg = g.new_output(nw, device=DEV), g.new_output(nw, device=DEV)
        L.check(pack(L.ptr(wdev), L.ptr(wf), L.ptr(wdg), Ct.byref(d), _stream()), "pack")
        yd = g.new_output(N, Ho, Wo, Co, device=DEV)
        assert fwd(L.ptr(xd), L.ptr(wf), L.ptr(yd), Ct.byref(d), L.ptr(ws), wsz, _stream()) == rc, "fwd"
        dx = g.new_output(N, H, W, C, device=DEV)
        assert dgrad(L.ptr(gyd), L.ptr(wdg), L.ptr(dx), Ct.byref(d), 0, L.ptr(ws), wsz, _stream()) == rc, "dgrad"
        dw = g.new_output(KS * KS * C, Co, device=DEV)
        assert wgrad(L.ptr(xd), L.ptr(gyd), L.ptr(dw), Ct.byref(d), L.ptr(ws), wsz, _stream()) == rc, "wgrad"
        return {"y": yd, "dx": dx, "dw": dw}
    got = run_direct(lambda g: run(g, g.workspace(need // 4, DEV)))
    tag = "contract: %sconv %dx%dx%dx%d->%d k%d s%d" % ("bf16 path " if bf16 else "", N, H, W, C, Co, KS, stride)
    if bf16:
        bounds = ((2e-5, 2e-5), (2e-5, 2e-5), (max(1e-4 * np.sqrt(N), 4e-6 * float(wref.abs().max())), 1e-4))
    elif cls:
        bounds = ((2e-5, 2e-5), (2e-5, 2e-5), (1e-4 * np.sqrt(N), 1e-4))
    else:
        bounds = ((2e-5, 1e-5), (2e-5, 1e-5), (1e-4, 1e-5))
    _report(tag + " fwd", got["y"].permute(0, 3, 1, 2), y, *bounds[0])
    _report(tag + " dgrad", got["dx"].permute(0, 3, 1, 2), x.grad, *bounds[1])
    _report(tag + " wgrad", got["dw"], wref, *bounds[2])
    null = run(Guard(NAN), None)
    g = Guard(NAN, short=True)
    short = run(g, g.workspace(need // 4, DEV))
    assert g.workspaces[0][2] * 4 == need - 4
    for k in null:
        assert torch.equal(short[k], null[k]), k
    g.outputs.clear()
    g.assert_untouched()
    g = Guard(NAN, offset=1)                       # the scratch 4 bytes off its alignment: AVVAD_EINVAL from all three, y / dx / dw
    run(g, g.workspace(need // 4, DEV), rc=-1)     # keep their poison (the packs before them were written, as they must be)
    g.outputs[:] = g.outputs[-3:]
    g.assert_untouched()


# =========================================================================================== fusion and losses
@pytest.mark.parametrize("training", [True, False])
def test_mcb_fusion_fn(training, monkeypatch):
    """McbFusionFn at B = 3, T = 4 (the size of test_av_net_mcb_fusion_vs_oracle) against the oracle's fusion.mcb +
    fusion.mcb_post, at the suite's output bound 1e-4, _report_grad for the gradients and that test's bound on the running
    variance.  The train-mode gradients are where an unordered bucket sum showed: 0.5 / sqrt(|y|) of the signed square root
    turns a last-bit difference of a small y into 2e-4 of d/d audio; with the ordered sums the fills agree bit for bit."""
    from oracle import fusion
    ops = _ops()
    rng = np.random.RandomState(5)
    h1, h2 = T(rng.randint(0, 1024, 513)), T(rng.randint(0, 1024, 512))
    s1 = T((2 * rng.randint(0, 2, 513) - 1).astype(np.float32))
    s2 = T((2 * rng.randint(0, 2, 512) - 1).astype(np.float32))
    a, v, G = stategen.rand(61, 3, 4, 513), stategen.rand(62, 3, 4, 512), stategen.rand(63, 3, 4, 1024)
    bw, bb = stategen.rand(64, 1024) * 0.5 + 1.0, stategen.rand(65, 1024)
    # eval mode divides by sqrt(running_var): the L2-normalised values are ~ 1e-2, a variance of ~ 1e-2 brings them to ~ 0.1
    rm0, rv0 = stategen.rand(66, 1024) * 1e-3, stategen.rand(67, 1024).abs() * 1e-2 + 1e-3
    eps, mom = 1e-8, 0.1
    ar, vr = a.clone().requires_grad_(True), v.clone().requires_grad_(True)
    bwr, bbr = bw.clone().requires_grad_(True), bb.clone().requires_grad_(True)
    rm_ref, rv_ref = rm0.clone(), rv0.clone()
    ref = fusion.mcb_post(fusion.mcb(ar, vr, h1, s1, h2, s2, 1024), bwr, bbr, rm_ref, rv_ref, eps, training, mom)
    (ref * G).sum().backward()
    dev = lambda t: t.to(DEV)
    h1d, s1d, h2d, s2d, gd = dev(h1), dev(s1), dev(h2), dev(s2), dev(G)

    def case():
        ag, vg = dev(a).requires_grad_(True), dev(v).requires_grad_(True)
        wg, bg = dev(bw).requires_grad_(True), dev(bb).requires_grad_(True)
        rm, rv = dev(rm0), dev(rv0)
        y = ops.McbFusionFn.apply(ag, vg, h1d, s1d, h2d, s2d, wg, bg, rm, rv, eps, training, mom)
        (y * gd).sum().backward()
        return {"y": y, "da": ag.grad, "dv": vg.grad, "dw": wg.grad, "db": bg.grad, "rm": rm, "rv": rv}
    got = _contract(monkeypatch, case)
    _backward_refused(monkeypatch, "avvad_mcb_fusion_bwd",
                      lambda: ops.McbFusionFn.apply(dev(a).requires_grad_(True), dev(v).requires_grad_(True), h1d, s1d, h2d, s2d,
                                                    dev(bw).requires_grad_(True), dev(bb).requires_grad_(True), dev(rm0), dev(rv0), eps,
                                                    training, mom),
                      lambda y: (y * gd).sum().backward())
    tag = "contract: McbFusionFn %s" % ("train" if training else "eval")
    _report(tag + " out", got["y"], ref, 1e-4)
    for k, r in (("da", ar), ("dv", vr), ("dw", bwr), ("db", bbr)):
        _report_grad(tag + " " + k, got[k], r.grad)
    _report(tag + " running_var", got["rv"], rv_ref, 1e-6, 1e-4)
    _report(tag + " running_mean", got["rm"], rm_ref, 1e-6, 1e-4)


def test_count_sketch_and_compact_bilinear_pooling(monkeypatch):
    """test_count_sketch_and_compact_bilinear_pooling_modules: the sketch against the reference's own output (golden
    ``misc``), the pooled vector and both input gradients against the oracle's FFT form.  No workspace: outputs only."""
    from oracle import fusion
    from packages.models.compact_bilinear_pooling import CompactBilinearPooling, CountSketch
    g = load_golden("misc")
    cs = CountSketch(513, 1024, T(g["cs_h"]), T(g["cs_s"])).to(DEV)
    xd, cg = T(g["cs_x"]).to(DEV), T(g["cs_g"]).to(DEV)
    rng = np.random.RandomState(5)
    h1, h2 = T(rng.randint(0, 1024, 513)), T(rng.randint(0, 1024, 512))
    s1 = T((2 * rng.randint(0, 2, 513) - 1).astype(np.float32))
    s2 = T((2 * rng.randint(0, 2, 512) - 1).astype(np.float32))
    a, v, G = stategen.rand(61, 2, 3, 513), stategen.rand(62, 2, 3, 512), stategen.rand(63, 2, 3, 1024)
    ar, vr = a.clone().requires_grad_(True), v.clone().requires_grad_(True)
    ref = fusion.mcb(ar, vr, h1, s1, h2, s2, 1024)
    (ref * G).sum().backward()
    m = CompactBilinearPooling(513, 512, 1024, h1, s1, h2, s2).to(DEV)
    ad, vd, gd = a.to(DEV), v.to(DEV), G.to(DEV)

    def case():
        x = xd.clone().requires_grad_(True)
        y = cs(x)
        (y * cg).sum().backward()
        ag, vg = ad.clone().requires_grad_(True), vd.clone().requires_grad_(True)
        out = m(ag, vg)
        (out * gd).sum().backward()
        return {"cs_y": y, "cs_dx": x.grad, "cbp": out, "cbp_dx": ag.grad, "cbp_dy": vg.grad}
    got = _contract(monkeypatch, case, short=None)
    _report("contract: CountSketch.forward vs reference", got["cs_y"], g["cs_y"], 1e-6)
    _report("contract: CountSketch backward vs reference", got["cs_dx"], g["cs_dx"], 1e-6)
    _report("contract: CompactBilinearPooling.forward", got["cbp"], ref, 2e-4, 1e-5)
    _report_grad("contract: CompactBilinearPooling d/dx", got["cbp_dx"], ar.grad)
    _report_grad("contract: CompactBilinearPooling d/dy", got["cbp_dy"], vr.grad)


def test_losses_and_layout_helpers(monkeypatch):
    """masked_bce on the ragged audio golden (loss and d/dlogits: rows t >= length get NO gradient, so the kernel must
    write their zeros itself), Bce2ClassesFn on the ``misc`` golden, ConcatColsFn and TransposeLast2Fn against torch."""
    from oracle import head
    ops = _ops()
    g = load_golden("audio_l2_h16")
    lens = g["lengths"].tolist()
    logits, tgt = T(g["y"]).to(DEV), T(g["target"]).to(DEV)
    lr = T(g["y"]).clone().requires_grad_(True)
    ref_loss = head.batch_loss(lr, T(g["target"]), lens, 1e-8)
    (ref_loss * 3.0).backward()
    mg = load_golden("misc")
    r1d, r2d, x2d = T(mg["bce2_r1"]).to(DEV), T(mg["bce2_r2"]).to(DEV), T(mg["bce2_x"]).to(DEV)
    ca, cb = stategen.rand(81, 3, 5, 513), stategen.rand(82, 3, 5, 512)
    tr = stategen.rand(83, 3, 37, 70)
    cad, cbd, trd = ca.to(DEV), cb.to(DEV), tr.to(DEV)
    gcat, gtr = stategen.rand(84, 3, 5, 1025).to(DEV), stategen.rand(85, 3, 70, 37).to(DEV)

    def case():
        lg = logits.clone().requires_grad_(True)
        loss = ops.masked_bce(lg, tgt, torch.LongTensor(lens), 1e-8)
        (loss * 3.0).backward()
        r1, r2 = r1d.clone().requires_grad_(True), r2d.clone().requires_grad_(True)
        l2 = ops.Bce2ClassesFn.apply(r1, r2, x2d, 1e-8)
        (l2 * 3.0).backward()
        a, b = cad.clone().requires_grad_(True), cbd.clone().requires_grad_(True)
        cat = ops.ConcatColsFn.apply(a, b)
        (cat * gcat).sum().backward()
        t = trd.clone().requires_grad_(True)
        tt = ops.TransposeLast2Fn.apply(t)
        (tt * gtr).sum().backward()
        return {"loss": loss, "dlogits": lg.grad, "bce2": l2, "d1": r1.grad, "d2": r2.grad, "cat": cat, "da": a.grad, "db": b.grad,
                "tt": tt, "dt": t.grad}
    got = _contract(monkeypatch, case, short=None)
    _report("contract: masked_bce loss", got["loss"], ref_loss.detach(), 1e-4)            # test_audio_net_golden
    _report("contract: masked_bce loss vs golden", got["loss"], g["loss"], 1e-4)
    _report("contract: masked_bce d/dlogits", got["dlogits"], lr.grad, 1e-6)               # test_bce_and_metrics
    _report("contract: bce_2classes", got["bce2"], mg["bce2"], 1e-6)                       # test_bce_2classes_vs_reference
    _report("contract: bce_2classes d/dr1", got["d1"], 3.0 * mg["bce2_d1"], 1e-6, 1e-5)
    _report("contract: bce_2classes d/dr2", got["d2"], 3.0 * mg["bce2_d2"], 1e-6, 1e-5)
    assert torch.equal(got["cat"].cpu(), torch.cat([ca, cb], 2))                           # copies: exact
    assert torch.equal(got["da"], gcat[..., :513]) and torch.equal(got["db"], gcat[..., 513:])
    assert torch.equal(got["tt"].cpu(), tr.transpose(1, 2)) and torch.equal(got["dt"], gtr.transpose(1, 2))


# =========================================================================================== front-end
def test_stft_modes_and_complex(monkeypatch):
    """test_stft_frontend_gpu at L = 4096 + 768 (the end-pad branch): modes 0 / 1 on a batch of two, the legacy mode 2 and
    stft_complex against the oracle's torch.stft restatement."""
    from oracle import frontend
    ops = _ops()
    Ln = 4096 + 768
    x = stategen.rand(90, Ln, scale=0.3)
    x = x / x.abs().max()
    xb = torch.stack([x, x.flip(0) * 0.5])
    ref = frontend.stft(x, fs=16e3, wlen_sec=64e-3, hop_percent=0.25, center=False, pad_at_end=True)        # (F, T, 2)
    refs = [frontend.stft(r, fs=16e3, wlen_sec=64e-3, hop_percent=0.25, center=False) for r in xb]
    pw_ref = torch.stack([(s ** 2).sum(-1).t() for s in refs])
    xd, xbd = x.to(DEV), xb.to(DEV)

    def case():
        return {"m0": ops.stft(xbd, mode=0), "m1": ops.stft(xbd, mode=1), "m2": ops.stft(xd, mode=2), "cplx": ops.stft_complex(xbd)}
    got = _contract(monkeypatch, case, short_ops={"avvad_stft mode 0": lambda: ops.stft(xbd, mode=0), "avvad_stft mode 2": lambda: ops.stft(xd, mode=2),
                                                  "avvad_stft_complex": lambda: ops.stft_complex(xbd)})
    _report("contract: stft mode 2 re/im", got["m2"], ref, 5e-4)
    _report("contract: stft mode 1 power", got["m1"], pw_ref, 2e-3, 1e-4)
    _report("contract: stft mode 0 log-power", torch.exp(got["m0"]) - 1e-8, pw_ref, 2e-3, 1e-4)
    _report("contract: stft_complex", got["cplx"], torch.stack([s.permute(1, 0, 2) for s in refs]), 5e-4)


def test_standardize_peak_normalize_and_peak(monkeypatch):
    """standardize with per-bin and with scalar statistics (test_input_standardisation_in_the_train_loop's inputs and
    bound), peak (exact, as test_streamed_features_vs_oracle asserts it) and peak_normalize: one float32 division of
    values that end up within [-1, 1], against a float64 quotient rounded once -- a reciprocal-and-multiply differs from
    it by at most one more rounding, 2 * 2^-24.  That bound is NEW, set here from the number format: no parity test of
    peak_normalize existed to take one from."""
    from oracle import frontend
    ops = _ops()
    a, v = stategen.rand(71, 3, 5, 513), stategen.rand(72, 3, 5, 67 * 67)
    am, as_ = stategen.rand(73, 513, 1), stategen.rand(74, 513, 1).abs() + 0.5
    vm, vs = torch.tensor([[0.4]]), torch.tensor([[2.5]])
    w = stategen.rand(75, 3, 5003, scale=0.3)
    dev = lambda t: t.to(DEV)
    ad, vd, amd, asd, vmd, vsd, wd = (dev(t) for t in (a, v, am, as_, vm, vs, w))

    def case():
        return {"audio": ops.standardize(ad, amd, asd), "video": ops.standardize(vd, vmd, vsd), "peak": ops.peak(wd),
                "norm": ops.peak_normalize(wd)}
    got = _contract(monkeypatch, case, short=None)
    _report("contract: standardise audio", got["audio"], frontend.standardize(a, am, as_), 1e-6, 1e-6)
    _report("contract: standardise video", got["video"], (v - vm.T) / (vs + 1e-8).T, 1e-6, 1e-6)
    assert torch.equal(got["peak"].cpu(), w.abs().max(dim=1).values)
    q = (w.double() / w.abs().max(dim=1, keepdim=True).values.double())
    _report("contract: peak_normalize", got["norm"], q, 2.0 ** -23)


def test_istft_and_resynth_ragged(monkeypatch):
    """The ragged batches of test_istft_gpu.py: the PARITY batches (64 / 16 with a one-frame row, 1024 / 256 with 260 rows
    over the engine's tiles) whose padding frames hold NaN, by _check_row; the fused round trip of
    test_round_trip_returns_the_waveform by its own bound."""
    import istft_ref as R
    from test_istft_gpu import _batch, _check_row, _covered
    from test_istft_gpu import _report as _ireport
    ops = _ops()
    batches = [(n_fft, hop, frames) + _batch(n_fft, hop, frames, seed=n_fft + hop) for n_fft, hop, frames in ((64, 16, [9, 4, 1]), (1024, 256, [130, 5]))]
    n_fft, hop, lens = 1024, 256, [5000, 5120, 3000]
    rng = np.random.default_rng(11)
    x = np.zeros((3, 5120), dtype=np.float32)
    for b, n in enumerate(lens):
        v = rng.standard_normal(n)
        x[b, :n] = v / np.abs(v).max()
    xd = T(x).to(DEV)

    def case():
        out = {"istft%d" % i: ops.istft(spec, nf, hp, n_frames=frames) for i, (nf, hp, frames, _, spec) in enumerate(batches)}
        out["resynth"] = ops.resynth(xd, None, mask_mode=0, n_fft=n_fft, hop=hop, sample_lengths=lens)
        return out
    nf0, hp0, frames0, _, spec0 = batches[0]
    got = _contract(monkeypatch, case, short_ops={
        "avvad_istft": lambda: ops.istft(spec0, nf0, hp0, n_frames=frames0),
        "avvad_resynth": lambda: ops.resynth(xd, None, mask_mode=0, n_fft=n_fft, hop=hop, sample_lengths=lens)})
    for i, (nf, hp, frames, rows, _) in enumerate(batches):
        Lmax = R.istft_length(max(frames), nf, hp)
        for b, S in enumerate(rows):
            natural = R.istft_length(frames[b], nf, hp)
            assert torch.count_nonzero(got["istft%d" % i][b, natural:]).item() == 0
            _check_row("contract %d/%d row %d" % (nf, hp, b), got["istft%d" % i][b], S.astype(np.complex128), nf, hp, length=Lmax)
    y = got["resynth"].cpu().numpy()
    for b, n in enumerate(lens):
        assert not y[b, n:].any()
        natural = R.istft_length(ops.n_frames(n, n_fft, hop), n_fft, hop)
        g32, ref = _covered(R.istft32_gemm(R.stft32_gemm(x[b, :n], n_fft, hop), n_fft, hop), x[b], n, natural, hop)
        e32 = float(np.abs(g32 - ref).max())
        gotb, ref = _covered(y[b], x[b], n, natural, hop)
        _ireport("contract: round trip L = %d" % n, gotb, ref, R.FACTOR * e32)


# =========================================================================================== statistics, labels, video
def test_statistics(monkeypatch):
    """stft_stats, accumulate_stats and finalize_stats on test_stats_gpu.py's ragged fixture batch, by
    test_reduction_is_exact_against_the_features_of_stft: the accumulators against a float64 host reduction of the
    features ``ops.stft`` returns (1e-12 relative), mean / std within one float32 of the float64 finalisation.  The
    accumulators are state (``zeros``): the workspaces and the mean / std outputs are what is poisoned."""
    import stats_ref as R
    from test_stats_gpu import F, FRAMES, adjacent, host_reduction, ragged_batch
    ops = _ops()
    wave, lens = ragged_batch()
    x = ops.stft(wave, mode=0)
    want = host_reduction(x, FRAMES)

    def case():
        acc = ops.stft_stats(ops.stats_new(F, DEV), wave, lens)
        acc2 = ops.accumulate_stats(ops.stats_new(F, DEV), x, FRAMES)
        mean, std = ops.finalize_stats(acc)
        return {"acc": acc, "acc2": acc2, "mean": mean, "std": std}
    got = _contract(monkeypatch, case, short_ops={"avvad_stft_stats": lambda: ops.stft_stats(ops.stats_new(F, DEV), wave, lens),
                                                  "avvad_stats_accumulate": lambda: ops.accumulate_stats(ops.stats_new(F, DEV), x, FRAMES)})
    for k in ("acc", "acc2"):
        a = got[k].cpu().numpy()
        assert a[-1] == want[-1] == 485
        assert (np.abs(a[:F] - want[:F]) / np.abs(want[:F])).max() <= 1e-12, k
        assert (np.abs(a[F:2 * F] - want[F:2 * F]) / want[F:2 * F]).max() <= 1e-12, k
    m64, s64 = R.finalize(want)
    assert adjacent(got["mean"].cpu().numpy(), m64.astype(np.float32)) and adjacent(got["std"].cpu().numpy(), s64.astype(np.float32))


def test_speech_targets_and_ibm_from_spectrum(monkeypatch):
    """VAD, IBM and robust IBM labels of utt_sa1_clean against the reference's own results (golden ``targets``) outside the
    stated rounding bands, as test_vad_matches_reference_and_restatement / test_ibm_both_layouts_match_reference do, and of
    test_targets_gpu.py's five-utterance ragged batch (a silent, an all-zero and a one-frame utterance): frames past a
    row's count are zero.  ibm_from_spectrum reads the legacy (F, T, 2) spectrum."""
    import target_ref as R
    from test_targets_cpu import CFGS, ibm_band, sa1, vad_band
    from test_targets_gpu import five_utterances, spectrum64
    ops = _ops()
    g = load_golden("targets")
    x = sa1("clean")
    xd = T(x).to(DEV).view(1, -1)
    utts = five_utterances()
    lens = [u.numel() for u in utts]
    wave = torch.zeros(len(utts), max(lens))
    for i, u in enumerate(utts):
        wave[i, :lens[i]] = u
    wd = wave.to(DEV)
    legacy = ops.stft(xd[0], mode=2)                                                     # (F, T, 2)

    def case():
        out = {}
        for tag, w, n in (("sa1", xd, [x.size]), ("five", wd, lens)):
            out[tag + "_vad"] = ops.speech_targets(w, n, "vad_labels")[1]
            out[tag + "_ibm"] = ops.speech_targets(w, n, "ibm_labels")[1]
            out[tag + "_rob"] = ops.speech_targets(w, n, "ibm_labels", robust=True)[1]
        out["spec_ibm"] = ops.ibm_from_spectrum(legacy)
        return out
    got = _contract(monkeypatch, case, short_ops={
        "avvad_target_vad": lambda: ops.speech_targets(wd, lens, "vad_labels"),
        "avvad_target_ibm": lambda: ops.speech_targets(wd, lens, "ibm_labels"),
        "avvad_target_ibm robust": lambda: ops.speech_targets(wd, lens, "ibm_labels", robust=True),
        "avvad_target_ibm_from_spectrum": lambda: ops.ibm_from_spectrum(legacy)})
    E, c = R.vad_energy(x, **CFGS["c64f"])
    vband = vad_band(E, c)
    v = got["sa1_vad"].cpu().numpy()[0, :, 0].astype(bool)
    assert np.array_equal(v[~vband], g["vad_clean_c64f"][0].astype(bool)[~vband])
    _, mag, M, tau = R.ibm_parts(spectrum64(x), 1e-8, 50)
    band = ibm_band(mag, M, tau)
    assert band.sum() <= 0.002 * band.size
    for k in ("sa1_ibm", "spec_ibm"):
        m = got[k].cpu().numpy()
        m = (m[0].T if k == "sa1_ibm" else m).astype(bool)
        assert np.array_equal(m[~band], g["ibm50_clean"].astype(bool)[~band]), k
    rob = got["sa1_rob"].cpu().numpy()[0].T.astype(bool)
    excl = band | vband[None, :]
    assert np.array_equal(rob[~excl], g["robust_clean"].astype(bool)[~excl])
    frames = [ops.target_frames(n)[1] for n in lens]
    for k in ("five_vad", "five_ibm", "five_rob"):
        t = got[k]
        assert bool(torch.isfinite(t).all()) and bool(((t == 0) | (t == 1)).all()), k
        for i, n in enumerate(frames):
            assert not t[i, n:].any(), (k, i)
    assert not got["five_vad"][3].any()                                                 # the all-zero utterance


def test_lip_decode(monkeypatch):
    """lip_decode on a ragged batch with the frame counts of the reference's data (golden ``lip_frames``: N and the label
    count that caps the output), unquantised, against tests/lip_ref.py at test_lip_gpu.py's tolerance; frames past a row's
    length are zero."""
    import lip_ref as R
    from test_lip_gpu import NPIX, tolerance
    ops = _ops()
    z = load_golden("lip_frames")
    n_in = [int(n) for n in z["n_in"][:3]]
    n_out = [int(n) for n in z["label_frames"][:3]]
    utts = [R.synthetic_coef(n, seed=3 + b, scale=1.0 + 11.0 * b) for b, n in enumerate(n_in)]
    padded = np.zeros((3, max(n_in), NPIX), np.float32)
    for b, u in enumerate(utts):
        padded[b, :n_in[b]] = u
        padded[b, n_in[b]:] = 1e6 * (b + 1)
    cd = T(padded).to(DEV)

    def case():
        video, lens = ops.lip_decode(cd, n_in, n_out=n_out, quantize=False)
        quant, _ = ops.lip_decode(cd, n_in, n_out=n_out)
        assert lens.tolist() == [min(ops.lip_out_frames(n), m) for n, m in zip(n_in, n_out)]
        return {"video": video, "quant": quant}
    got = _contract(monkeypatch, case)
    for b, u in enumerate(utts):
        ref = R.decode(u, n_out=n_out[b], quantize=False)
        tol = tolerance(u)
        err = np.abs(got["video"][b, :ref.shape[0]].cpu().numpy().astype(np.float64) - ref).max()
        print("contract: lip_decode row %d: max |gpu - float64| = %.3e level, tolerance %.3e" % (b, err, tol))
        assert err <= tol
        for k in ("video", "quant"):
            assert not got[k][b, ref.shape[0]:].any()
        q = got["quant"][b, :ref.shape[0]].cpu().numpy().astype(np.float64)
        differ = q != R.quantise(ref)
        assert np.all((np.abs(ref - np.rint(ref)) <= tol)[differ]) and np.all(np.abs(q - R.quantise(ref))[differ] == 1.0)


# =========================================================================================== streaming
def test_lstm_stack_state_two_chunks(monkeypatch):
    """lstm_stack_state over two consecutive chunks of a ragged batch from a random state, against torch.nn.LSTM on the
    CPU (test_lstm_state_vs_torch's reference and bounds).  The state tensors are state; workspace, y and the fresh
    (h_n, c_n) are poisoned.  B = 17 and H = 64: two sequence groups, the vector form."""
    from test_stream_gpu import _torch_lstm_rows
    ops = _ops()
    B, H, In, Tc = 17, 64, 40, 3
    torch.manual_seed(B * 7919 + H + In)
    lstm = torch.nn.LSTM(In, H, 2)
    x = torch.randn(B, 2 * Tc, In)
    h0, c0 = torch.randn(2, B, H) * 0.5, torch.randn(2, B, H)
    rng = random.Random(B + H)
    lens = [rng.randint(0, 2 * Tc) for _ in range(B)]
    lens[0], lens[-1] = 2 * Tc, 0
    ry, rh, rc = _torch_lstm_rows(lstm, x, lens, h0, c0)
    gl = lstm.to(DEV)
    xd, hd, cd = x.to(DEV), h0.to(DEV), c0.to(DEV)

    def case():
        ys, state = [], (hd, cd)
        for t0 in (0, Tc):
            ln = [min(max(l - t0, 0), Tc) for l in lens]
            y, state = ops.lstm_stack_state(xd[:, t0:t0 + Tc].contiguous(), ln, gl, state=state)
            ys.append(y)
        return {"y": torch.cat(ys, 1), "h": state[0], "c": state[1]}
    got = _contract(monkeypatch, case)
    assert torch.equal(hd.cpu(), h0) and torch.equal(cd.cpu(), c0)
    _report("contract: lstm_stack_state y", got["y"], ry, 1e-4)
    _report("contract: lstm_stack_state h_n", got["h"], rh, 1e-4)
    _report("contract: lstm_stack_state c_n", got["c"], rc, 1e-4, 1e-5)


@pytest.mark.parametrize("name,cuts,k", [("wn_nobias", [5 + 11 + 71, 71 * 3], 71), ("wn_w0_t16", [2047 + 256 * 3, 256 * 13], 256)])
def test_wavenet_stream_two_chunks(name, cuts, k, monkeypatch):
    """The streaming encoder over two consecutive chunks (the warm-up lies in the first) against the reference's own y:
    test_encoder_nobias_golden_streamed (the direct form) and test_encoder_w0_golden_streamed (the MFMA form)."""
    from avvad.stream import FrameClock
    from test_stream_gpu import _encoder_from_golden
    ops = _ops()
    g = load_golden(name)
    enc = _encoder_from_golden(g)
    x = T(g["x"]).to(DEV)
    ref = T(g["y"]).permute(0, 2, 1)
    assert sum(cuts) == x.shape[2]
    B = x.shape[0]

    def case():
        clock = FrameClock(B, enc.receptive_field, k)
        state = ops.wavenet_stream_state(enc, B, x.device)
        outs, s0 = [], 0
        for n in cuts:
            frames, used = clock.advance([n] * B)
            outs.append(ops.wavenet_stream(x[:, :, s0:s0 + n].contiguous(), [n] * B, used, enc, state, k, max(frames)))
            s0 += n
        return {"y": torch.cat(outs, 1), "state": state}
    got = _contract(monkeypatch, case)
    _report("contract: %s streamed in two chunks vs the reference's y" % name, got["y"], ref, 1e-4)


def test_stft_stream_two_chunks(monkeypatch):
    """stft_stream over two consecutive chunks of two rows (the second call final) against the whole-utterance ``ops.stft``
    features at test_stft_stream_gpu.py's feature bound and the oracle; the basis, the features and the spare state are
    outputs and poisoned, the state is state.  The entry point takes no workspace."""
    from avvad.stream import SampleClock
    from oracle import frontend
    ops = _ops()
    x = stategen.rand(91, 2, 6000, scale=0.3)
    x = x / x.abs().max(dim=1, keepdim=True).values
    xd = x.to(DEV)
    refs = [frontend.log_power(frontend.stft(r, wlen_sec=64e-3, hop_percent=0.25, center=False, pad_at_end=True)).transpose(0, 1) for r in x]

    def case():
        basis = ops.stft_stream_basis(1024, DEV)
        clock = SampleClock(2, 1024, 256)
        state = ops.stft_stream_state(2, 1024, DEV)
        f1, n1 = ops.stft_stream(xd[:, :2500].contiguous(), None, clock, state, basis)
        f2, n2 = ops.stft_stream(xd[:, 2500:].contiguous(), None, clock, state, basis, final=[0, 1])
        assert n1 == [n1[0]] * 2 and n2 == [n2[0]] * 2
        return {"feat": torch.cat([f1[:, :n1[0]], f2[:, :n2[0]]], 1), "basis": basis, "state": state}
    got = _contract(monkeypatch, case, short=None)
    assert got["feat"].shape[1] == refs[0].shape[0] == ops.n_frames(6000, 1024, 256)
    for b in range(2):
        _report("contract: stft_stream row %d vs oracle" % b, got["feat"][b], refs[b], 2e-3, 1e-4)


# =========================================================================================== pointer alignment
def test_alignment_gemm_operands(monkeypatch):
    """gemm.hip picks 16-byte fetches for A (RowVec4, ColPlain<4>) and B (ColPlain<4>) from the base pointer: shapes
    whose leading dimensions allow the vector form, once aligned and once with A and B re-homed 4 bytes off."""
    ops = _ops()
    for M, N, K, tA, tB in ((37, 132, 96, 0, 0), (132, 64, 40, 1, 0), (128, 128, 64, 0, 1)):
        A, B, bias, ref = _gemm_operands(M, N, K, tA, tB)
        for off in (0, 1):
            a, b, bs = _rehome(T(A).to(DEV), off), _rehome(T(B).to(DEV), off), T(bias).to(DEV)
            with guarded(monkeypatch, ops, NAN) as g:
                c = _out(M, N)
                ops.gemm(a, b, c, M, N, K, A.shape[1], B.shape[1], N, bool(tA), bool(tB), bias=bs)
                g.check()
            _report("alignment: gemm %dx%dx%d tA%d tB%d, A / B at +%d bytes" % (M, N, K, tA, tB, 4 * off), c, ref + bias,
                    1e-5 * np.sqrt(K) * 4)


def test_alignment_adam_step():
    """avvad_adam_step (FlatAdam's kernel) with n = 1001, not a multiple of 4: the float4 kernel plus a scalar tail when
    all four pointers are 16-byte aligned, the scalar kernel for everything when they are not; three steps against
    torch.optim.Adam at test_adam_matches_torch's bound.  Values behind n must not change."""
    from avvad import _lib as L
    n = 1001
    torch.manual_seed(1)
    p0 = torch.randn(n)
    grads = [torch.randn(n) for _ in range(3)]
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-3, betas=(0.9, 0.999))
    for gq in grads:
        ref.grad = gq.clone()
        opt.step()
    for off in (0, 1):
        bufs = [torch.full((n + off + 64,), 7.0, device=DEV) for _ in range(4)]
        p, gr, m, v = (b[off:off + n] for b in bufs)
        p.copy_(p0.to(DEV)); m.zero_(); v.zero_()
        assert p.data_ptr() % 16 == 4 * off
        for step, gq in enumerate(grads, 1):
            gr.copy_(gq.to(DEV))
            L.check(L.lib().avvad_adam_step(L.ptr(p), L.ptr(gr), L.ptr(m), L.ptr(v), n, 1e-3, 0.9, 0.999, 1e-8, step, _stream()), "adam")
        _report("alignment: adam n=1001 at +%d bytes" % (4 * off), p, ref.detach(), 1e-6)
        for b in bufs:
            assert bool((b[:off] == 7.0).all()) and bool((b[off + n:] == 7.0).all())


def test_alignment_speech_targets_and_ibm_from_spectrum(monkeypatch):
    """target.hip picks vector loads of ``wave`` and vector stores of ``vad`` / ``ibm`` / ``out`` from the pointers: the
    labels of utt_sa1_clean with everything aligned and with the waveform (and, for ibm_from_spectrum, the vad factor)
    re-homed 4 bytes off, against the reference's results outside the rounding bands."""
    import target_ref as R
    from test_targets_cpu import CFGS, ibm_band, sa1, vad_band
    from test_targets_gpu import spectrum64
    ops = _ops()
    g = load_golden("targets")
    x = sa1("clean")
    x = x[:len(x) // 4 * 4]                       # L % 4 == 0: the vector form needs it as well
    E, c = R.vad_energy(x, **CFGS["c64f"])
    vband = vad_band(E, c)
    _, mag, M, tau = R.ibm_parts(spectrum64(x), 1e-8, 50)
    band = ibm_band(mag, M, tau)
    vref = (E > c * E.min())
    iref = (mag > tau)
    for off in (0, 1):
        xd = _rehome(T(x).to(DEV), off).view(1, -1)
        with guarded(monkeypatch, ops, NAN) as gd:
            vad = ops.speech_targets(xd, [x.size], "vad_labels")[1]
            ibm = ops.speech_targets(xd, [x.size], "ibm_labels")[1]
            spec = ops.stft(xd[0], mode=2)
            frame_vad = _rehome(vad.reshape(-1), off)
            sib = ops.ibm_from_spectrum(spec, vad=frame_vad)
            gd.check()
        v = vad.cpu().numpy()[0, :, 0].astype(bool)
        assert np.array_equal(v[~vband], vref[~vband]), off
        m = ibm.cpu().numpy()[0].T.astype(bool)
        assert np.array_equal(m[~band], iref[~band]), off
        s = sib.cpu().numpy().astype(bool)
        excl = band | vband[None, :]
        assert np.array_equal(s[~excl], (iref & vref[None, :])[~excl]), off
    # the OUTPUT pointers 4 bytes off (``ops`` allocates its own, aligned): the same three entry points through the C ABI,
    # each against the aligned run above bit for bit (the store form changes no value) with the floats around it intact
    from avvad import _lib as L
    lib = L.lib()
    w2, d, ws, cnt, _ = ops._target_call(xd, [x.size], 16e3, 64e-3, 0.25, False, "reflect", True, 1.70, 1e-8, 50)
    Tn, Fn = d.T, d.n_fft // 2 + 1

    def off_out(*shape):
        n = int(np.prod(shape))
        buf = torch.full((n + 8,), 7.0, device=DEV)
        return buf, buf[1:1 + n].view(shape)
    vb, vo = off_out(1, Tn, 1)
    L.check(lib.avvad_target_vad(L.ptr(w2), L.ptr(cnt[0]), L.ptr(cnt[1]), L.ptr(vo), Ct.byref(d), L.ptr(ws), ws.numel() * 4, _stream()), "vad")
    ib, io = off_out(1, Tn, Fn)
    L.check(lib.avvad_target_ibm(L.ptr(w2), L.ptr(cnt[0]), L.ptr(cnt[1]), 0, L.ptr(io), Ct.byref(d), L.ptr(ws), ws.numel() * 4, _stream()), "ibm")
    sb, so = off_out(Fn, Tn)
    d1 = L.TargetDesc(1, Tn, 2 * (Fn - 1), 1, Tn, 0, 1e-8, 1.0, float(ops.np_power10(-50 / 20.0)))
    ws2 = torch.empty(2, device=DEV)
    L.check(lib.avvad_target_ibm_from_spectrum(L.ptr(spec), spec.stride(1), spec.stride(0), L.ptr(frame_vad), L.ptr(so), Ct.byref(d1),
                                               L.ptr(ws2), 8, _stream()), "ibm_from_spectrum")
    assert vo.data_ptr() % 16 == 4 and torch.equal(vo, vad) and torch.equal(io, ibm) and torch.equal(so, sib)
    for buf, view in ((vb, vo), (ib, io), (sb, so)):
        assert float(buf[0]) == 7.0 and bool((buf[1 + view.numel():] == 7.0).all())


def test_alignment_lstm_w_hh(monkeypatch):
    """The recurrent weights 4 bytes off: the forward leaves its fused step / persistent kernels (they read W_hh rows 16
    bytes at a time) for the GEMM + gate kernels, the backward its fused form (lstm.hip: ``bwd_form``), and the state layer
    takes its scalar form (stream.hip: ``vec``).  Each against the oracle / torch at the aligned form's bound."""
    import torch.nn as nn
    from oracle import head
    from test_stream_gpu import _torch_lstm_rows
    ops = _ops()
    B, H, Tn, In = 16, 256, 5, 40
    torch.manual_seed(B + H)
    lstm = nn.LSTM(In, H, 1)
    x = torch.randn(B, Tn, In)
    lens = [int(v) for v in torch.randint(1, Tn + 1, (B,))]
    lens[0], lens[1] = Tn, 1
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in lstm.state_dict().items()}
    xr = x.clone().requires_grad_(True)
    ref = head.lstm_stack(xr, lens, sd, "", 1)
    Gd = torch.randn(B, Tn, H)
    (ref * Gd).sum().backward()
    h0, c0 = torch.randn(1, B, H) * 0.5, torch.randn(1, B, H)
    ry, rh, rc = _torch_lstm_rows(lstm, x, lens, h0, c0)
    lstm = lstm.to(DEV)
    for off in (0, 1):
        with torch.no_grad():
            lstm.weight_hh_l0.data = _rehome(lstm.weight_hh_l0.data, off)
        assert lstm.weight_hh_l0.data_ptr() % 16 == 4 * off
        for p in lstm.parameters():
            p.grad = None
        xg = x.to(DEV).requires_grad_(True)
        with guarded(monkeypatch, ops, NAN) as g:
            y = ops.lstm_stack(xg, lens, lstm)
            (y * Gd.to(DEV)).sum().backward()
            ys, (hn, cn) = ops.lstm_stack_state(x.to(DEV), lens, lstm, state=(h0.to(DEV), c0.to(DEV)))
            g.check()
        tag = "alignment: lstm w_hh at +%d bytes" % (4 * off)
        _report(tag + " forward", y, ref, 1e-4)
        _report_grad(tag + " d/dx", xg.grad, xr.grad)
        for k, p in lstm.named_parameters():
            _report_grad(tag + " d/d" + k, p.grad, sd[k].grad)
        _report(tag + " state layer y", ys, ry, 1e-4)
        _report(tag + " state layer h_n", hn, rh, 1e-4)
        _report(tag + " state layer c_n", cn, rc, 1e-4, 1e-5)


def test_alignment_stft_wave(monkeypatch):
    """``wave[3:]`` of a longer buffer through stft (modes 0 and 2): the framing reads rows that start anywhere."""
    from oracle import frontend
    ops = _ops()
    Ln = 4096 + 768
    x = stategen.rand(90, Ln, scale=0.3)
    x = x / x.abs().max()
    ref = frontend.stft(x, fs=16e3, wlen_sec=64e-3, hop_percent=0.25, center=False, pad_at_end=True)
    pw_ref = (ref ** 2).sum(-1).t()[None]
    for off in (0, 3):
        xd = _rehome(x.to(DEV), off)
        with guarded(monkeypatch, ops, NAN) as g:
            m2, m0 = ops.stft(xd, mode=2), ops.stft(xd, mode=0)
            g.check()
        _report("alignment: stft re/im, wave at +%d bytes" % (4 * off), m2, ref, 5e-4)
        _report("alignment: stft log-power, wave at +%d bytes" % (4 * off), torch.exp(m0) - 1e-8, pw_ref, 2e-3, 1e-4)


def test_misaligned_workspace_is_refused_before_any_launch(monkeypatch):
    """Pointer class "workspace": 16-byte aligned.  Every entry point that takes one returns AVVAD_EINVAL for a workspace
    4 bytes off and launches nothing (guards, workspace and outputs keep their poison)."""
    import torch.nn as nn
    import istft_ref  # noqa: F401  (test_istft_gpu's helper module must be importable)
    from packages.models.wavenet_autoencoder import wavenet_autoencoder
    from test_istft_gpu import _batch
    from test_stats_gpu import F
    ops = _ops()
    torch.manual_seed(0)
    lstm = nn.LSTM(40, 32, 1).to(DEV)
    xl = torch.randn(3, 4, 40, device=DEV)
    g = load_golden("wn_tiny")
    wn = wavenet_autoencoder(**wn_cfg_from(g))
    wn.load_state_dict({k[2:]: T(v) for k, v in g.items() if k.startswith("p.")})
    wn = wn.to(DEV).eval()
    xw = T(g["x"]).to(DEV)
    wave = torch.randn(2, 4096 + 768, device=DEV) * 0.1
    feats, legacy = ops.stft(wave, mode=0), ops.stft(wave[0], mode=2)
    _, spec = _batch(64, 16, [9, 4], seed=1, fill=0.0)
    coef = torch.randn(1, 3, 67 * 67, device=DEV)
    from avvad import nn as avnn
    from packages.models.Video_Net import DeepVAD_video
    vm = DeepVAD_video(2, 16, 1)
    vm.load_state_dict(_video_state())
    vm = vm.to(DEV).eval()
    frames = stategen.rand(21, 2, 67, 67).to(DEV)
    rng = np.random.RandomState(5)
    h1, h2 = T(rng.randint(0, 1024, 513)).to(DEV), T(rng.randint(0, 1024, 512)).to(DEV)
    s1, s2 = torch.ones(513, device=DEV), torch.ones(512, device=DEV)
    bn = [torch.ones(1024, device=DEV), torch.zeros(1024, device=DEV), torch.zeros(1024, device=DEV), torch.ones(1024, device=DEV)]
    a, v = torch.randn(1, 2, 513, device=DEV), torch.randn(1, 2, 512, device=DEV)
    cases = {
        "gemm": lambda: ops.gemm(xl.view(12, 40), lstm.weight_ih_l0, _out(12, 128), 12, 128, 40, 40, 40, 128, transB=True),
        "lstm": lambda: ops.lstm_stack(xl, [4, 1, 2], lstm),
        "lstm state": lambda: ops.lstm_stack_state(xl, [4, 1, 2], lstm),
        "wavenet": lambda: wn(xw),
        "wavenet stream": lambda: ops.wavenet_stream(xw[:, :, :8].contiguous(), [8] * xw.shape[0], [0] * xw.shape[0], wn,
                                                     ops.wavenet_stream_state(wn, xw.shape[0], DEV), 4, 2),
        "trunk": lambda: avnn.trunk_forward(vm.features, frames, False),
        "mcb": lambda: ops.McbFusionFn.apply(a, v, h1, s1, h2, s2, bn[0], bn[1], bn[2], bn[3], 1e-8, False, 0.1),
        "stft": lambda: ops.stft(wave, mode=0),
        "stft_complex": lambda: ops.stft_complex(wave),
        "istft": lambda: ops.istft(spec, 64, 16, n_frames=[9, 4]),
        "resynth": lambda: ops.resynth(wave, None, mask_mode=0),
        "stft_stats": lambda: ops.stft_stats(ops.stats_new(F, DEV), wave, [4096 + 768, 3000]),
        "target vad": lambda: ops.speech_targets(wave, [4096 + 768, 3000], "vad_labels"),
        "target ibm": lambda: ops.speech_targets(wave, [4096 + 768, 3000], "ibm_labels"),
        "lip_decode": lambda: ops.lip_decode(coef, [3]),
        "accumulate_stats": lambda: ops.accumulate_stats(ops.stats_new(F, DEV), feats),
        "ibm_from_spectrum": lambda: ops.ibm_from_spectrum(legacy),
    }
    for name, case in cases.items():
        try:
            expect_refused(monkeypatch, ops, case, "AVVAD_EINVAL", offset=1)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
        case()                                    # (and the same call with torch's own, aligned blocks goes through)


def test_misaligned_coef_basis_and_accumulators_are_refused():
    """The other pointers the header wants aligned, through the C ABI with a pointer 4 bytes off: lip_decode's ``coef``
    (16), the stft_stream basis (16) and the float64 statistics accumulators (8) return AVVAD_EINVAL; the outputs and
    accumulators keep their contents."""
    from avvad import _lib as L
    from test_stats_gpu import F
    ops = _ops()
    lib = L.lib()
    off4 = lambda t: Ct.c_void_p(t.data_ptr() + 4)
    # statistics accumulators
    x = torch.randn(2, 5, F, device=DEV)
    accbuf = torch.zeros(2 * F + 2, dtype=torch.float64, device=DEV)
    ws = torch.full(((lib.avvad_stats_workspace(10, F) + 3) // 4,), NAN, device=DEV)
    rc = lib.avvad_stats_accumulate(L.ptr(x), None, off4(accbuf), 2, 5, F, F, L.ptr(ws), ws.numel() * 4, _stream())
    assert rc == -1 and not accbuf.any() and bool(torch.isnan(ws).all())
    mean, std = torch.full((F,), NAN, device=DEV), torch.full((F,), NAN, device=DEV)
    assert lib.avvad_stats_finalize(off4(accbuf), F, L.ptr(mean), L.ptr(std), _stream()) == -1
    assert bool(torch.isnan(mean).all()) and bool(torch.isnan(std).all())
    wave = torch.randn(1, 4096, device=DEV)
    d = L.StftDesc(1, 4096, 1024, 256, 13, 1e-8)
    ws = torch.full(((lib.avvad_stft_stats_workspace(Ct.byref(d)) + 3) // 4,), NAN, device=DEV)
    cnt = torch.tensor([13], dtype=torch.int32, device=DEV)
    assert lib.avvad_stft_stats(L.ptr(wave), L.ptr(cnt), off4(accbuf), Ct.byref(d), L.ptr(ws), ws.numel() * 4, _stream()) == -1
    assert not accbuf.any() and bool(torch.isnan(ws).all())
    # the streaming basis: building it and using it
    nb = lib.avvad_stft_stream_basis_bytes(1024) // 4
    bbuf = torch.full((nb + 4,), NAN, device=DEV)
    assert lib.avvad_stft_stream_basis(1024, off4(bbuf), _stream()) == -1 and bool(torch.isnan(bbuf).all())
    basis = ops.stft_stream_basis(1024, DEV)
    bbuf[1:1 + nb].copy_(basis)
    chunk = torch.randn(1, 2048, device=DEV)
    from avvad.stream import SampleClock
    frames, pending, pad = SampleClock(1, 1024, 256).advance([2048])
    assert frames == [5]
    counts = torch.tensor([[2048], pending, frames, pad], dtype=torch.int32, device=DEV)
    state, new = torch.zeros(1, 1024, device=DEV), torch.full((1, 1024), NAN, device=DEV)
    out = torch.full((1, 5, 513), NAN, device=DEV)
    sd = L.StftStreamDesc(1, 2048, 1024, 256, 5, 5, 1e-8, 1e-8)
    args = lambda b: (L.ptr(chunk), L.ptr(counts[0]), L.ptr(counts[1]), L.ptr(counts[2]), L.ptr(counts[3]), None, L.ptr(state), L.ptr(new),
                      b, None, None, L.ptr(out), Ct.byref(sd), _stream())
    assert lib.avvad_stft_stream_fwd(*args(off4(bbuf))) == -1
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(new).all())
    assert lib.avvad_stft_stream_fwd(*args(L.ptr(basis))) == 0 and bool(torch.isfinite(out).all())
    # lip_decode's coefficients
    cbuf = torch.randn(3 * 67 * 67 + 4, device=DEV)
    ld = L.LipDesc(1, 3, 3, 6, 67, 67, 25, 12, 1, 1e-8)
    ws = torch.full(((lib.avvad_lip_decode_workspace(Ct.byref(ld)) + 3) // 4,), NAN, device=DEV)
    idx = torch.tensor([[0], [3], [6], [0]], dtype=torch.int32, device=DEV)
    video = torch.full((1, 6, 67, 67), NAN, device=DEV)
    largs = lambda c: (c, L.ptr(idx[0]), L.ptr(idx[1]), None, L.ptr(video), L.ptr(idx[3]), None, None, None, Ct.byref(ld), L.ptr(ws),
                       ws.numel() * 4, _stream())
    assert lib.avvad_lip_decode(*largs(off4(cbuf))) == -1
    assert bool(torch.isnan(video).all()) and bool(torch.isnan(ws).all())
    assert lib.avvad_lip_decode(*largs(L.ptr(cbuf))) == 0 and bool(torch.isfinite(video).all())
