"""torch.autograd wrappers around the C ABI of libavvad_hip.so.

PyTorch is plumbing here: it owns device memory, streams and the autograd tape;
every arithmetic step of the hot path runs in the HIP kernels.  All tensors
must be fp32, contiguous and live on the GPU -- anything else raises.
"""
import ctypes as C
import math
import os

import torch

from . import _lib as L
from ._lib import AvvadError         # by name too: target_frames takes the utterance length as ``L``


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_SIDE = {}


_SIDE_PRIO = int(os.environ.get("AVVAD_SIDE_PRIO", "-1"))      # read once at import
_OVERLAP = os.environ.get("AVVAD_OVERLAP", "1") != "0"


def side_stream():
    """The per-device side HIP stream on which independent sub-graphs (the audio encoder) run next to the main one."""
    dev = torch.cuda.current_device()
    if dev not in _SIDE:
        _SIDE[dev] = torch.cuda.Stream(device=dev, priority=_SIDE_PRIO)
    return _SIDE[dev]


def side_streams():
    return list(_SIDE.values())


_FORK = {}        # device -> the stream that forked work onto the side stream (DeepVAD_AV.forward's caller stream)


def note_fork(main):
    _FORK[torch.cuda.current_device()] = main


def _join_side_after_backward():
    """Called from a Function.backward that ran on the side stream and wrote parameter gradients IN PLACE.  autograd
    joins the streams of a backward pass through its AccumulateGrad nodes; gradients written in place bypass those, so
    the engine never learns that the side stream took part and the caller's stream would NOT wait for it when
    backward() returns: an optimiser step (or a .cpu() of a gradient) could overtake the encoder's backward kernels.
    (Observed: bimodal 1e-7 differences between identical trainings of a tiny model -- Adam read the encoder's gradients
    before or after they were complete.)  The join is queued as an end-of-backward callback, so the trunk's backward on
    the main stream is not made to wait in the middle of the pass."""
    if not _SIDE:                 # no side stream was ever created (audio-only / video-only models, CPU-side unit tests)
        return
    dev = torch.cuda.current_device()
    side = _SIDE.get(dev)
    if side is None or torch.cuda.current_stream() != side:
        return
    main = _FORK.get(dev) or torch.cuda.default_stream()
    torch.autograd.Variable._execution_engine.queue_callback(lambda: main.wait_stream(side))


def overlap_enabled():
    return _OVERLAP


def set_overlap(flag):
    """Run the audio encoder on the side stream (True, default) or in line on the current stream."""
    global _OVERLAP
    _OVERLAP = bool(flag)


def _dev(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.AvvadError("%s must be a GPU tensor: the AV-VAD hot path has no CPU fallback "
                           "(use the oracle/ package for CPU checks)" % name)
    if t.dtype != torch.float32:
        raise L.AvvadError("%s must be float32, got %s" % (name, t.dtype))
    return t.contiguous()


def _wave2d(wave):
    """wave (B, L) or (L,) on the GPU -> (the tensor as given, its (B, L) view)"""
    w = _dev(wave, "wave")
    return w, (w.view(1, -1) if w.dim() == 1 else w)


def _ints(v, B=None, hi=None, msg=None, default=None, what=None):
    """Host list of ints from a tensor or a sequence: THE per-row list check.  With ``msg``, or ``what`` (the argument's
    name, for the usual message, made only when it is needed): B values within 0..hi (``hi`` None: no upper bound), or
    AvvadError.  With ``default``: None stands for B times that value."""
    if v is None and default is not None:
        return [default] * B
    vals = [int(x) for x in (v.tolist() if isinstance(v, torch.Tensor) else v)]
    if (msg or what) and (len(vals) != B or any(n < 0 or (hi is not None and n > hi) for n in vals)):
        raise L.AvvadError(msg or "%s must hold one value in [0, %s] per row (%d rows), got %s" % (what, hi, B, vals))
    return vals


def _mean_std(mean, std, F, msg=None):
    """the statistics as flat GPU vectors of F values each"""
    mean, std = _dev(mean, "mean").reshape(-1), _dev(std, "std").reshape(-1)
    if mean.numel() != F or std.numel() != F:
        raise L.AvvadError(msg or "mean / std must hold %d values" % F)
    return mean, std


def _ws(nbytes, device):
    if nbytes == 0:
        raise L.AvvadError("workspace query failed (bad descriptor)")
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)


# ---------------------------------------------------------------------------
# Direct gradient accumulation.  Every backward kernel ACCUMULATES (+=) into the gradient pointer it is
# given, so when a parameter already owns a gradient buffer (FlatAdam re-homes all of them into one flat
# buffer) the kernel writes there directly and the Function returns None for that input: no zero-fill, no
# temporary, no autograd add kernel per parameter (~300 tiny launches per step saved).  Because autograd's
# AccumulateGrad node is bypassed, its post-accumulate hooks do not fire: listeners (the DP bucket reducer)
# register in GRAD_SINKS and are told about every parameter written this way.
GRAD_SINKS = []


def _grad_target(p, needed):
    """-> (tensor to accumulate into or None, direct?)"""
    if not needed or p is None:
        return None, False
    g = getattr(p, "grad", None)
    if isinstance(p, torch.nn.Parameter) and g is not None and g.is_contiguous() and g.dtype == torch.float32:
        return g, True
    return torch.zeros_like(p), False


def _finish_grads(params, targets):
    """returned gradients for autograd (None where written in place) + sink notification"""
    out = []
    if any(direct for _, direct in targets):
        _join_side_after_backward()
    for p, (g, direct) in zip(params, targets):
        if direct:
            for sink in GRAD_SINKS:
                sink(p)
            out.append(None)
        else:
            out.append(g)
    return out


def lengths_i32(lengths, device):
    """`lengths` arrives as a LongTensor (train loop) or a Python list (eval)."""
    if isinstance(lengths, torch.Tensor):
        return lengths.to(device=device, dtype=torch.int32).contiguous()
    return torch.tensor([int(v) for v in lengths], dtype=torch.int32, device=device)


# --------------------------------------------------------------------------- GEMM / Linear
def engine_ws(device):
    """Scratch of the GEMM engine (partial tiles of its stream-K round): caller-allocated per call, like every
    workspace of the C ABI; torch's caching allocator makes that a pointer bump."""
    return torch.empty(L.lib().avvad_engine_workspace() // 4, dtype=torch.float32, device=device)


def gemm(A, B, C_out, M, N, K, lda, ldb, ldc, transA=False, transB=False, bias=None, accumulate=False, split_k=1):
    d = L.GemmDesc(M, N, K, lda, ldb, ldc, int(transA), int(transB), int(accumulate), split_k, 0, 0)
    ws = engine_ws(C_out.device)
    L.check(L.lib().avvad_gemm_f32(L.ptr(A), L.ptr(B), L.ptr(bias), L.ptr(C_out), C.byref(d), L.ptr(ws), ws.numel() * 4,
                                   _stream()), "avvad_gemm_f32")


class LinearFn(torch.autograd.Function):
    """y = x W^T + b   (nn.Linear: Audio_Net.py:59, Video_Net.py:116, AV_Net.py:140)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x2 = _dev(x, "x").view(-1, x.shape[-1])
        w = _dev(weight, "weight")
        rows, K = x2.shape
        N = w.shape[0]
        y = torch.empty(rows, N, dtype=torch.float32, device=x.device)
        gemm(x2, w, y, rows, N, K, K, K, N, transB=True, bias=_dev(bias, "bias") if bias is not None else None)
        ctx.save_for_backward(x2, w)
        ctx.has_bias = bias is not None
        ctx.prm = (weight, bias)
        return y.view(x.shape[:-1] + (N,))

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        rows, K = x2.shape
        N = w.shape[0]
        dy2 = _dev(dy, "dy").view(rows, N)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x2)
            gemm(dy2, w, dx, rows, K, N, N, K, K)                       # [rows,N] x [N,K]
            dx = dx.view(dy.shape[:-1] + (K,))
        tw = _grad_target(ctx.prm[0], ctx.needs_input_grad[1])
        tb = _grad_target(ctx.prm[1], ctx.has_bias and ctx.needs_input_grad[2])
        if tw[0] is not None:
            gemm(dy2, x2, tw[0], N, K, rows, N, K, K, transA=True, accumulate=True)   # dy^T x
        if tb[0] is not None:
            L.check(L.lib().avvad_colsum_acc(L.ptr(dy2), rows, N, L.ptr(tb[0]), _stream()), "avvad_colsum_acc")
        dw, db = _finish_grads(ctx.prm, (tw, tb))
        return dx, dw, db


# --------------------------------------------------------------------------- LSTM layer
class LstmLayerFn(torch.autograd.Function):
    """One unidirectional LSTM layer over a padded batch with packed-sequence semantics."""

    @staticmethod
    def forward(ctx, x, lens32, w_ih, w_hh, b_ih, b_hh):
        x = _dev(x, "x")
        B, T, In = x.shape
        H = w_hh.shape[1]
        w_ih, w_hh, b_ih, b_hh = (_dev(t, n) for t, n in ((w_ih, "w_ih"), (w_hh, "w_hh"), (b_ih, "b_ih"), (b_hh, "b_hh")))
        d = L.LstmDesc(B, T, In, H, lens32.data_ptr(), 1)
        ws = _ws(L.lib().avvad_lstm_workspace(C.byref(d)), x.device)
        y = torch.empty(B, T, H, dtype=torch.float32, device=x.device)
        L.check(L.lib().avvad_lstm_layer_fwd(L.ptr(x), L.ptr(w_ih), L.ptr(w_hh), L.ptr(b_ih), L.ptr(b_hh), L.ptr(y),
                                             C.byref(d), L.ptr(ws), ws.numel() * 4, _stream()), "avvad_lstm_layer_fwd")
        ctx.save_for_backward(x, lens32, w_ih, w_hh, y, ws)
        ctx.prm = (w_ih, w_hh, b_ih, b_hh)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, lens32, w_ih, w_hh, y, ws = ctx.saved_tensors
        B, T, In = x.shape
        H = w_hh.shape[1]
        dy = _dev(dy, "dy")
        d = L.LstmDesc(B, T, In, H, lens32.data_ptr(), 1)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        tg = [_grad_target(p, ctx.needs_input_grad[2 + i]) for i, p in enumerate(ctx.prm)]
        L.check(L.lib().avvad_lstm_layer_bwd(L.ptr(x), L.ptr(w_ih), L.ptr(w_hh), L.ptr(y), L.ptr(dy), L.ptr(dx),
                                             L.ptr(tg[0][0]), L.ptr(tg[1][0]), L.ptr(tg[2][0]), L.ptr(tg[3][0]), C.byref(d),
                                             L.ptr(ws), ws.numel() * 4, _stream()), "avvad_lstm_layer_bwd")
        dw_ih, dw_hh, db_ih, db_hh = _finish_grads(ctx.prm, tg)
        return dx, None, dw_ih, dw_hh, db_ih, db_hh


def lstm_stack(x, lengths, lstm_module):
    """Runs the parameters held by an ``nn.LSTM`` container through the HIP layers."""
    if lstm_module.bidirectional or not lstm_module.bias or lstm_module.proj_size:
        raise L.AvvadError("only the unidirectional, biased LSTM of the reference is supported")
    lens32 = lengths_i32(lengths, x.device)
    y = x
    for l in range(lstm_module.num_layers):
        y = LstmLayerFn.apply(y, lens32, getattr(lstm_module, "weight_ih_l%d" % l), getattr(lstm_module, "weight_hh_l%d" % l),
                              getattr(lstm_module, "bias_ih_l%d" % l), getattr(lstm_module, "bias_hh_l%d" % l))
    return y


# --------------------------------------------------------------------------- WaveNet encoder
class WavenetFn(torch.autograd.Function):
    """wave (B,qc,L) -> (B,Bn,P).  params: causal_w, causal_b, bott_w, bott_b, then per layer
    dil_w, dil_b, dense_w, dense_b (biases None when use_bias is False)."""

    @staticmethod
    def _desc(cfg, B, Lin, dil_arr, save):
        # shared_device: this call runs on the side stream next to the trunk's kernels (DeepVAD_AV with overlap)
        dev = torch.cuda.current_device()
        shared = _OVERLAP and dev in _SIDE and torch.cuda.current_stream() == _SIDE[dev]
        return L.WavenetDesc(B, Lin, cfg["quantization_channel"], cfg["en_residual_channel"], cfg["en_dilation_channel"],
                             cfg["en_bottleneck_width"], cfg["filter_width"], cfg["en_pool_kernel_size"],
                             len(cfg["dilations"]), dil_arr, int(cfg["use_bias"]), int(save), int(shared))

    @staticmethod
    def _ptrs(ts, n):
        cw, cb, bw, bb = ts[:4]
        rest = ts[4:]
        arrs = [L.ptr_array(rest[k::4][:n]) for k in range(4)]
        p = L.WavenetPtrs(L.ptr(cw), L.ptr(cb), arrs[0], arrs[1], arrs[2], arrs[3], L.ptr(bw), L.ptr(bb))
        return p, arrs  # keep arrs alive

    @staticmethod
    def forward(ctx, wave, cfg, *params):
        wave = _dev(wave, "wave")
        B, qc, Lin = wave.shape
        n = len(cfg["dilations"])
        if qc != cfg["quantization_channel"] or len(params) != 4 + 4 * n:
            raise L.AvvadError("wavenet: bad input channels / parameter list")
        ctx.owners = params          # the Parameter objects themselves (their .grad may be written directly)
        params = tuple(None if t is None else _dev(t, "param") for t in params)
        dil_arr = (C.c_int * max(1, n))(*cfg["dilations"])
        save = any(ctx.needs_input_grad)
        d = WavenetFn._desc(cfg, B, Lin, dil_arr, save)
        ws = _ws(L.lib().avvad_wavenet_workspace(C.byref(d)), wave.device)
        out = torch.empty(B, cfg["en_bottleneck_width"], cfg["en_pool_kernel_size"], dtype=torch.float32, device=wave.device)
        p, keep = WavenetFn._ptrs(params, n)
        L.check(L.lib().avvad_wavenet_fwd(L.ptr(wave), C.byref(p), L.ptr(out), C.byref(d), L.ptr(ws), ws.numel() * 4,
                                          _stream()), "avvad_wavenet_fwd")
        ctx.cfg = cfg
        ctx.save_for_backward(wave, ws, *[t for t in params if t is not None])
        ctx.mask = [t is not None for t in params]
        return out

    @staticmethod
    def backward(ctx, dout):
        cfg = ctx.cfg
        saved = ctx.saved_tensors
        wave, ws = saved[0], saved[1]
        it = iter(saved[2:])
        params = tuple(next(it) if m else None for m in ctx.mask)
        n = len(cfg["dilations"])
        B, qc, Lin = wave.shape
        dil_arr = (C.c_int * max(1, n))(*cfg["dilations"])
        d = WavenetFn._desc(cfg, B, Lin, dil_arr, True)
        owners = ctx.owners
        tg = [_grad_target(o if o is not None else t, t is not None and ctx.needs_input_grad[2 + i])
              for i, (o, t) in enumerate(zip(owners, params))]
        grads = tuple(g for g, _ in tg)
        dwave = torch.empty_like(wave) if ctx.needs_input_grad[0] else None
        p, keep1 = WavenetFn._ptrs(params, n)
        g, keep2 = WavenetFn._ptrs(grads, n)
        L.check(L.lib().avvad_wavenet_bwd(L.ptr(wave), C.byref(p), L.ptr(_dev(dout, "dout")), C.byref(g), L.ptr(dwave),
                                          C.byref(d), L.ptr(ws), ws.numel() * 4, _stream()), "avvad_wavenet_bwd")
        grads = tuple(_finish_grads([o if o is not None else t for o, t in zip(owners, params)], tg))
        return (dwave, None) + grads


# --------------------------------------------------------------------------- streaming inference (csrc/stream.hip)
def _lstm_check(lstm_module):
    if lstm_module.bidirectional or not lstm_module.bias or lstm_module.proj_size:
        raise L.AvvadError("only the unidirectional, biased LSTM of the reference is supported")


def lstm_stack_state(x, lengths, lstm_module, state=None, out=None):
    """The parameters of an ``nn.LSTM`` container over the next ``T`` steps of ``B`` independent rows, state in and out
    (inference only).  x (B,T,In); ``lengths`` per-row step counts in [0, T]: padded output steps are zero, a row's state
    stops at its length, length 0 passes it through bit for bit.  ``state`` = (h, c), each (num_layers, B, H) like
    torch's, or None for zeros; ``out`` = (h, c) tensors to receive the new state (may be ``state`` itself: in place),
    or None for fresh ones.  -> (y (B,T,H), (h_n, c_n))."""
    _lstm_check(lstm_module)
    x = _dev(x, "x")
    if x.dim() != 3:
        raise L.AvvadError("x must be (B, T, In), got %s" % (tuple(x.shape),))
    B, T, In = x.shape
    nl, H = lstm_module.num_layers, lstm_module.hidden_size
    if In != lstm_module.input_size or B < 1 or T < 1:
        raise L.AvvadError("x %s does not fit an LSTM with input size %d" % (tuple(x.shape), lstm_module.input_size))

    def pair(p, what):
        h, c = p
        for t in (h, c):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or \
                    tuple(t.shape) != (nl, B, H):
                raise L.AvvadError("%s must be two contiguous float32 GPU tensors of shape %s" % (what, (nl, B, H)))
        return h, c
    h0, c0 = pair(state, "state") if state is not None else (None, None)
    if out is not None:
        hn, cn = pair(out, "out")
    else:
        hn = torch.empty(nl, B, H, dtype=torch.float32, device=x.device)
        cn = torch.empty_like(hn)
    lens32 = lengths_i32(lengths, x.device)
    if lens32.numel() != B:
        raise L.AvvadError("lengths must have one entry per row")
    y = x
    with torch.no_grad():
        for l in range(nl):
            w_ih, w_hh, b_ih, b_hh = (_dev(getattr(lstm_module, "%s_l%d" % (n, l)), n)
                                      for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
            d = L.LstmDesc(B, T, y.shape[2], H, lens32.data_ptr(), 0)
            ws = _ws(L.lib().avvad_lstm_state_workspace(C.byref(d)), x.device)
            y_l = torch.empty(B, T, H, dtype=torch.float32, device=x.device)
            L.check(L.lib().avvad_lstm_layer_fwd_state(
                L.ptr(y), L.ptr(w_ih), L.ptr(w_hh), L.ptr(b_ih), L.ptr(b_hh), L.ptr(h0[l]) if h0 is not None else None,
                L.ptr(c0[l]) if c0 is not None else None, L.ptr(y_l), L.ptr(hn[l]), L.ptr(cn[l]), C.byref(d), L.ptr(ws),
                ws.numel() * 4, _stream()), "avvad_lstm_layer_fwd_state")
            y = y_l
    return y, (hn, cn)


def _stream_desc(enc, B, Lc):
    n = len(enc.dilations)
    dil_arr = (C.c_int * max(1, n))(*enc.dilations)
    d = L.WavenetDesc(B, Lc, enc.quantization_channel, enc.en_residual_channel, enc.en_dilation_channel,
                      enc.en_bottleneck_width, enc.filter_width, 1, n, dil_arr, int(enc.use_bias), 0, 0)
    return d, dil_arr


def wavenet_stream_state(enc, B, device):
    """Zeroed state blocks (B, floats) of the streaming encoder for ``B`` rows of the ``wavenet_autoencoder`` ``enc``:
    all zeros is "start of utterance"."""
    d, _keep = _stream_desc(enc, B, 1)
    nbytes = L.lib().avvad_wavenet_stream_state_bytes(C.byref(d))
    if nbytes == 0:
        raise L.AvvadError("streaming encoder: bad configuration")
    return torch.zeros(B, nbytes // 4, dtype=torch.float32, device=device)


def wavenet_stream(chunk, n_valid, skip, enc, state, k, out_frames):
    """The next samples of ``B`` rows through the encoder (inference only).  chunk (B,qc,n); ``n_valid`` / ``skip``
    per-row counts (lists or int32 GPU tensors): row b consumes n_valid[b] columns, drops its first skip[b] output
    columns (remaining warm-up) and averages the rest in frames of ``k`` columns.  ``state`` (from
    ``wavenet_stream_state``) is updated in place.  -> (B, out_frames, Bn), frame-major; frames a row does not fill are
    zero.  The caller keeps (n_valid - skip) % k == 0 wherever n_valid > skip (``avvad.stream`` does)."""
    chunk = _dev(chunk, "chunk")
    if chunk.dim() != 3 or chunk.shape[1] != enc.quantization_channel or chunk.shape[2] < 1:
        raise L.AvvadError("chunk must be (B, %d, n >= 1), got %s" % (enc.quantization_channel, tuple(chunk.shape)))
    B, _, Lc = chunk.shape
    d, _keep = _stream_desc(enc, B, Lc)
    nbytes = L.lib().avvad_wavenet_stream_state_bytes(C.byref(d))
    if not isinstance(state, torch.Tensor) or not state.is_cuda or state.dtype != torch.float32 or \
            not state.is_contiguous() or tuple(state.shape) != (B, nbytes // 4):
        raise L.AvvadError("state must be the contiguous float32 GPU tensor of wavenet_stream_state(enc, %d, device)" % B)
    nv, sk = lengths_i32(n_valid, chunk.device), lengths_i32(skip, chunk.device)
    if nv.numel() != B or sk.numel() != B:
        raise L.AvvadError("n_valid and skip must have one entry per row")
    params = [enc.en_causal_layer.weight, enc.en_causal_layer.bias, enc.bottleneck_layer.weight, enc.bottleneck_layer.bias]
    for dil, dense in zip(enc.en_dilation_layer_stack, enc.en_dense_layer_stack):
        params += [dil.weight, dil.bias, dense.weight, dense.bias]
    params = tuple(None if t is None else _dev(t.detach(), "param") for t in params)
    p, _keep2 = WavenetFn._ptrs(params, len(enc.dilations))
    ws = _ws(L.lib().avvad_wavenet_stream_workspace(C.byref(d)), chunk.device)
    out = torch.empty(B, int(out_frames), enc.en_bottleneck_width, dtype=torch.float32, device=chunk.device)
    L.check(L.lib().avvad_wavenet_stream_fwd(L.ptr(chunk), C.byref(p), L.ptr(state), L.ptr(nv), L.ptr(sk), int(k),
                                             L.ptr(out) if out.numel() else None, int(out_frames), C.byref(d), L.ptr(ws),
                                             ws.numel() * 4, _stream()), "avvad_wavenet_stream_fwd")
    return out


# --------------------------------------------------------------------------- ResNet-18 trunk
class TrunkFn(torch.autograd.Function):
    """frames (N,H,W) -> (N,512).  tensors: 20 conv_w, 20 bn_w, 20 bn_b, 20 running_mean, 20 running_var
    in the conv index order of include/avvad.h.  Running stats are updated in place when training."""

    @staticmethod
    def _params(ts):
        n = L.TRUNK_NCONV
        p = L.TrunkParams()
        for i in range(n):
            p.conv_w[i] = ts[i].data_ptr()
            p.bn_w[i] = ts[n + i].data_ptr()
            p.bn_b[i] = ts[2 * n + i].data_ptr()
            p.bn_rm[i] = ts[3 * n + i].data_ptr()
            p.bn_rv[i] = ts[4 * n + i].data_ptr()
        return p

    @staticmethod
    def forward(ctx, frames, training, momentum, eps, *ts):
        frames = _dev(frames, "frames")
        N, H, W = frames.shape
        n = L.TRUNK_NCONV
        if len(ts) != 5 * n:
            raise L.AvvadError("trunk: expected %d tensors" % (5 * n))
        owners = ts
        ts = tuple(_dev(t, "trunk tensor") for t in ts)
        save = any(ctx.needs_input_grad[4:4 + 3 * n])
        d = L.TrunkDesc(N, H, W, int(training), float(momentum), float(eps), int(save))
        ws = _ws(L.lib().avvad_trunk_workspace(C.byref(d)), frames.device)
        feat = torch.empty(N, 512, dtype=torch.float32, device=frames.device)
        p = TrunkFn._params(ts)
        L.check(L.lib().avvad_trunk_fwd(L.ptr(frames), C.byref(p), L.ptr(feat), C.byref(d), L.ptr(ws), ws.numel() * 4,
                                        _stream()), "avvad_trunk_fwd")
        if save:
            ctx.save_for_backward(frames, ws, *ts)
            ctx.cfg = (int(training), float(momentum), float(eps))
            ctx.bf16 = L.get_option("bf16") == 1          # the data path this forward ran (csrc/trunk.hip native_bf16)
            ctx.owners = owners
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        saved = ctx.saved_tensors
        frames, ws, ts = saved[0], saved[1], saved[2:]
        N, H, W = frames.shape
        n = L.TRUNK_NCONV
        training, momentum, eps = ctx.cfg
        d = L.TrunkDesc(N, H, W, training, momentum, eps, 1)
        p = TrunkFn._params(ts)
        g = L.TrunkGrads()
        tg = [_grad_target(ctx.owners[i], ctx.needs_input_grad[4 + i]) for i in range(3 * n)]
        for i, (gt, _) in enumerate(tg):
            if gt is not None:
                (g.conv_w, g.bn_w, g.bn_b)[i // n][i % n] = gt.data_ptr()
        L.check(L.lib().avvad_trunk_bwd(L.ptr(frames), C.byref(p), L.ptr(_dev(dfeat, "dfeat")), C.byref(g), C.byref(d),
                                        L.ptr(ws), ws.numel() * 4, _stream()), "avvad_trunk_bwd")
        grads = _finish_grads(ctx.owners[:3 * n], tg)
        return (None, None, None, None) + tuple(grads) + (None,) * (2 * n)


def _trunk_node(feat):
    """the TrunkFn node behind ``feat`` -> (frames, workspace, descriptor, whether its forward ran the bf16 data path)"""
    todo, seen, node = [feat.grad_fn], set(), None          # breadth-first over the autograd graph behind `feat`
    while todo:
        f = todo.pop(0)
        if f is None or f in seen:
            continue
        seen.add(f)
        if type(f).__name__ == "TrunkFnBackward":
            node = f
            break
        todo.extend(nf for nf, _ in f.next_functions)
    if node is None:
        raise L.AvvadError("no TrunkFn node behind this tensor (was the forward run with gradients enabled?)")
    frames, ws = node.saved_tensors[0], node.saved_tensors[1]
    N, H, W = frames.shape
    training, momentum, eps = node.cfg
    return frames, ws, L.TrunkDesc(N, H, W, training, momentum, eps, 1), bool(node.bf16)


def _trunk_slot(d, idx):
    off, c, h, w = C.c_size_t(), C.c_int(), C.c_int(), C.c_int()
    L.check(L.lib().avvad_trunk_activation(C.byref(d), idx, C.byref(off), C.byref(c), C.byref(h), C.byref(w)), "avvad_trunk_activation")
    return off.value, c.value, h.value, w.value


def trunk_saved_activations(feat):
    """Test support: the post-ReLU activations kept for backward by the TrunkFn node behind ``feat``, as a dict
    name -> (N,C,H,W) view: ``pool``, ``<stage>.<block>.a1``, ``<stage>.<block>`` (the oracle's names).  A forward that ran
    the bf16 data path (option "bf16" = 1) keeps them as NHWC bf16 at the same offsets, in the first half of each slot: they
    come back as exact float32 COPIES of the stored values."""
    frames, ws, d, bf16 = _trunk_node(feat)
    N = frames.shape[0]
    out = {}
    for idx in range(17):
        off, c, h, w = _trunk_slot(d, idx)
        if bf16:
            t = ws[off: off + N * h * w * c // 2].view(torch.bfloat16).view(N, h, w, c).permute(0, 3, 1, 2).float()
        else:
            t = ws[off: off + N * h * w * c].view(N, h, w, c).permute(0, 3, 1, 2)
        k = (idx - 1) // 2
        name = "pool" if idx == 0 else "%d.%d%s" % (4 + k // 2, k % 2, ".a1" if (idx - 1) % 2 == 0 else "")
        out[name] = t
    return out


def trunk_saved_pool_argmax(feat):
    """Test support: the max pool's arg-max plane kept for backward by the TrunkFn node behind ``feat``: (N,64,h2,w2) uint8,
    the window position dh*3+dw (first maximum in row-major scan order) of every pooled element.  Like the activations it
    must be read before ``backward()``, which frees the workspace."""
    frames, ws, d, _ = _trunk_node(feat)
    N = frames.shape[0]
    off, c, h, w = _trunk_slot(d, 17)
    words = ws[off: off + N * h * w * (c // 4)]
    return words.view(torch.uint8).view(N, h, w, c).permute(0, 3, 1, 2)       # (little endian: byte k of word q = channel 4q+k)


# --------------------------------------------------------------------------- MCB fusion
class McbFusionFn(torch.autograd.Function):
    """audio (B,T,A), video (B,T,V) -> BatchNorm1d(L2norm(ssqrt(MCB(audio, video))))  (B,T,D)  (AV_Net.py:109-121)."""

    @staticmethod
    def forward(ctx, audio, video, h1, s1, h2, s2, bn_w, bn_b, rm, rv, eps, training, momentum):
        audio, video = _dev(audio, "audio"), _dev(video, "video")
        B, T, A = audio.shape
        V = video.shape[-1]
        D = bn_w.numel()
        for t, n in ((h1, "h1"), (h2, "h2")):
            if not t.is_cuda or t.dtype != torch.long:
                raise L.AvvadError("%s must be an int64 GPU tensor" % n)
        d = L.McbDesc(B * T, A, V, D, float(eps), int(training), float(momentum), 1)
        ws = _ws(L.lib().avvad_mcb_workspace(C.byref(d)), audio.device)
        out = torch.empty(B, T, D, dtype=torch.float32, device=audio.device)
        L.check(L.lib().avvad_mcb_fusion_fwd(L.ptr(audio), L.ptr(video), L.ptr(h1), L.ptr(_dev(s1, "s1")), L.ptr(h2),
                                             L.ptr(_dev(s2, "s2")), L.ptr(_dev(bn_w, "bn_w")), L.ptr(_dev(bn_b, "bn_b")),
                                             L.ptr(rm), L.ptr(rv), L.ptr(out), C.byref(d), L.ptr(ws), ws.numel() * 4,
                                             _stream()), "avvad_mcb_fusion_fwd")
        ctx.save_for_backward(audio, video, h1, s1, h2, s2, bn_w, ws)
        ctx.cfg = (float(eps), int(training), float(momentum))
        ctx.prm = (bn_w, bn_b)
        return out

    @staticmethod
    def backward(ctx, dout):
        audio, video, h1, s1, h2, s2, bn_w, ws = ctx.saved_tensors
        B, T, A = audio.shape
        V, D = video.shape[-1], bn_w.numel()
        eps, training, momentum = ctx.cfg
        d = L.McbDesc(B * T, A, V, D, eps, training, momentum, 1)
        da = torch.empty_like(audio) if ctx.needs_input_grad[0] else None
        dv = torch.empty_like(video) if ctx.needs_input_grad[1] else None
        tg = [_grad_target(ctx.prm[0], ctx.needs_input_grad[6]), _grad_target(ctx.prm[1], ctx.needs_input_grad[7])]
        L.check(L.lib().avvad_mcb_fusion_bwd(L.ptr(audio), L.ptr(video), L.ptr(h1), L.ptr(s1), L.ptr(h2), L.ptr(s2),
                                             L.ptr(bn_w), L.ptr(_dev(dout, "dout")), L.ptr(da), L.ptr(dv), L.ptr(tg[0][0]),
                                             L.ptr(tg[1][0]), C.byref(d), L.ptr(ws), ws.numel() * 4, _stream()),
                "avvad_mcb_fusion_bwd")
        dw, db = _finish_grads(ctx.prm, tg)
        return da, dv, None, None, None, None, dw, db, None, None, None, None, None


class CountSketchFn(torch.autograd.Function):
    """psi(x, h, s): out[..., h[i]] += s[i] x[..., i]  (compact_bilinear_pooling.py:7-27,41-57)."""

    @staticmethod
    def forward(ctx, h, s, output_size, x):
        x = _dev(x, "x")
        if not h.is_cuda or h.dtype != torch.long:
            raise L.AvvadError("h must be an int64 GPU tensor")
        In = x.shape[-1]
        rows = x.numel() // In
        out = torch.empty(x.shape[:-1] + (output_size,), dtype=torch.float32, device=x.device)
        L.check(L.lib().avvad_count_sketch_fwd(L.ptr(x), L.ptr(h), L.ptr(_dev(s, "s")), L.ptr(out), rows, In, output_size,
                                               _stream()), "avvad_count_sketch_fwd")
        ctx.save_for_backward(h, s)
        ctx.dims = (tuple(x.shape), rows, In, output_size)
        return out

    @staticmethod
    def backward(ctx, dout):
        h, s = ctx.saved_tensors
        shape, rows, In, D = ctx.dims
        dx = torch.empty(shape, dtype=torch.float32, device=dout.device)
        L.check(L.lib().avvad_count_sketch_bwd(L.ptr(_dev(dout, "dout")), L.ptr(h), L.ptr(s), L.ptr(dx), rows, In, D, _stream()),
                "avvad_count_sketch_bwd")
        return None, None, None, dx


class CompactBilinearPoolingFn(torch.autograd.Function):
    """psi(x,h1,s1) (*) psi(y,h2,s2): the raw pooled vector (compact_bilinear_pooling.py:140-220)."""

    @staticmethod
    def forward(ctx, h1, s1, h2, s2, output_size, x, y):
        x, y = _dev(x, "x"), _dev(y, "y")
        if x.shape[:-1] != y.shape[:-1]:
            raise L.AvvadError("compact bilinear pooling: leading dimensions differ")
        for t, n in ((h1, "h1"), (h2, "h2")):
            if not t.is_cuda or t.dtype != torch.long:
                raise L.AvvadError("%s must be an int64 GPU tensor" % n)
        A, V = x.shape[-1], y.shape[-1]
        rows = x.numel() // A
        out = torch.empty(x.shape[:-1] + (output_size,), dtype=torch.float32, device=x.device)
        L.check(L.lib().avvad_mcb_fwd(L.ptr(x), L.ptr(y), L.ptr(h1), L.ptr(_dev(s1, "s1")), L.ptr(h2), L.ptr(_dev(s2, "s2")),
                                      L.ptr(out), rows, A, V, output_size, _stream()), "avvad_mcb_fwd")
        ctx.save_for_backward(h1, s1, h2, s2, x, y)
        ctx.dims = (rows, A, V, output_size)
        return out

    @staticmethod
    def backward(ctx, dout):
        h1, s1, h2, s2, x, y = ctx.saved_tensors
        rows, A, V, D = ctx.dims
        dx = torch.empty_like(x) if ctx.needs_input_grad[5] else None
        dy = torch.empty_like(y) if ctx.needs_input_grad[6] else None
        L.check(L.lib().avvad_mcb_bwd(L.ptr(x), L.ptr(y), L.ptr(h1), L.ptr(s1), L.ptr(h2), L.ptr(s2), L.ptr(_dev(dout, "dout")),
                                      L.ptr(dx), L.ptr(dy), rows, A, V, D, _stream()), "avvad_mcb_bwd")
        return None, None, None, None, None, dx, dy


# --------------------------------------------------------------------------- loss
class Bce2ClassesFn(torch.autograd.Function):
    """-mean(sum(x log(r1+eps) + (1-x) log(r2+eps), dim=-1))  (models/utils.py:115-116), r1/r2 probabilities."""

    @staticmethod
    def forward(ctx, r1, r2, x, eps):
        r1, r2 = _dev(r1, "r1"), _dev(r2, "r2")
        x = _dev(x.to(torch.float32), "x")
        if r1.shape != r2.shape or r1.shape != x.shape:
            raise L.AvvadError("binary_cross_entropy_2classes: r1, r2, x must have the same shape")
        Y = r1.shape[-1]
        rows = r1.numel() // Y
        loss = torch.empty(1, dtype=torch.float32, device=r1.device)
        d1, d2 = torch.empty_like(r1), torch.empty_like(r2)
        L.check(L.lib().avvad_bce_2classes(L.ptr(r1), L.ptr(r2), L.ptr(x), L.ptr(loss), L.ptr(d1), L.ptr(d2), rows, Y, float(eps),
                                           _stream()), "avvad_bce_2classes")
        ctx.save_for_backward(d1, d2)
        return loss.view(())

    @staticmethod
    def backward(ctx, dloss):
        out = []
        for g in ctx.saved_tensors:
            g = g.clone()
            L.check(L.lib().avvad_scale_by_device_scalar(L.ptr(g), L.ptr(_dev(dloss, "dloss").view(1)), g.numel(), _stream()),
                    "avvad_scale_by_device_scalar")
            out.append(g)
        return out[0], out[1], None, None



class MaskedBceFn(torch.autograd.Function):
    """sum_b mean_{t<len_b} BCE-with-eps(logits, targets)  (models/utils.py:108-113 + train_AV_net.py:298-301)."""

    @staticmethod
    def forward(ctx, logits, targets, lens32, eps):
        logits = _dev(logits, "logits")
        targets = _dev(targets.to(torch.float32), "targets")
        B, T, Y = logits.shape
        loss = torch.empty(1, dtype=torch.float32, device=logits.device)
        dl = torch.empty_like(logits)
        L.check(L.lib().avvad_bce_masked(L.ptr(logits), L.ptr(targets), L.ptr(lens32), L.ptr(loss), L.ptr(dl), B, T, Y,
                                         float(eps), _stream()), "avvad_bce_masked")
        ctx.save_for_backward(dl)
        return loss.view(())

    @staticmethod
    def backward(ctx, dloss):
        (dl,) = ctx.saved_tensors
        g = dl.clone()
        L.check(L.lib().avvad_scale_by_device_scalar(L.ptr(g), L.ptr(_dev(dloss, "dloss").view(1)), g.numel(), _stream()),
                "avvad_scale_by_device_scalar")
        return g, None, None, None


def masked_bce(logits, targets, lengths, eps=1e-8):
    return MaskedBceFn.apply(logits, targets, lengths_i32(lengths, logits.device), eps)


# --------------------------------------------------------------------------- layout helpers
class ConcatColsFn(torch.autograd.Function):
    """torch.cat([a, b], dim=2) (AV_Net.py:124), each branch written straight into the buffer."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _dev(a, "a"), _dev(b, "b")
        rows = a.numel() // a.shape[-1]
        ca, cb = a.shape[-1], b.shape[-1]
        y = torch.empty(a.shape[:-1] + (ca + cb,), dtype=torch.float32, device=a.device)
        lib = L.lib()
        L.check(lib.avvad_copy_cols(L.ptr(a), L.ptr(y), rows, ca, ca, 0, ca + cb, 0, _stream()), "avvad_copy_cols")
        L.check(lib.avvad_copy_cols(L.ptr(b), L.ptr(y), rows, cb, cb, 0, ca + cb, ca, _stream()), "avvad_copy_cols")
        ctx.dims = (rows, ca, cb, a.shape, b.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        rows, ca, cb, sa, sb = ctx.dims
        dy = _dev(dy, "dy")
        lib = L.lib()
        da = db = None
        if ctx.needs_input_grad[0]:
            da = torch.empty(sa, dtype=torch.float32, device=dy.device)
            L.check(lib.avvad_copy_cols(L.ptr(dy), L.ptr(da), rows, ca, ca + cb, 0, ca, 0, _stream()), "avvad_copy_cols")
        if ctx.needs_input_grad[1]:
            db = torch.empty(sb, dtype=torch.float32, device=dy.device)
            L.check(lib.avvad_copy_cols(L.ptr(dy), L.ptr(db), rows, cb, ca + cb, ca, cb, 0, _stream()), "avvad_copy_cols")
        return da, db


class TransposeLast2Fn(torch.autograd.Function):
    """(B,C,T) -> (B,T,C): encoder output to the LSTM's batch-first layout."""

    @staticmethod
    def forward(ctx, x):
        x = _dev(x, "x")
        B, Cc, T = x.shape
        y = torch.empty(B, T, Cc, dtype=torch.float32, device=x.device)
        L.check(L.lib().avvad_transpose_last2(L.ptr(x), L.ptr(y), B, Cc, T, _stream()), "avvad_transpose_last2")
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _dev(dy, "dy")
        B, T, Cc = dy.shape
        dx = torch.empty(B, Cc, T, dtype=torch.float32, device=dy.device)
        L.check(L.lib().avvad_transpose_last2(L.ptr(dy), L.ptr(dx), B, T, Cc, _stream()), "avvad_transpose_last2")
        return dx


# --------------------------------------------------------------------------- STFT front-end (no gradient)
def _end_pad(L, fs, wlen_sec, hop_percent):
    """The reference appends one hop of zeros when the utterance is not a whole number of hops -- by this test, in its
    floats and its order of divisions (packages/processing/stft.py:134-139, target.py:28-46)."""
    v = L / fs / wlen_sec / hop_percent
    return math.ceil(v) != int(v)


def n_frames(L, n_fft, hop, pad_at_end=True, fs=16e3):
    """frame count of stft_pytorch(center=False): one hop of zeros is appended when the utterance is not a whole
    number of hops (packages/processing/stft.py:134-139)."""
    if pad_at_end and _end_pad(L, fs, n_fft / fs, hop / n_fft):
        L = L + hop
    return (L - n_fft) // hop + 1


def stft(wave, n_fft=1024, hop=256, mode=0, eps=1e-8, pad_at_end=True, fs=16e3, mean=None, std=None, norm_eps=1e-8):
    """wave (B,L) or (L,) on the GPU.  mode 0: log-power (B,T,F); 1: power (B,T,F); 2: legacy real view (F,T,2).
    With ``mean`` / ``std`` (F values each, mode 0) the train-set standardisation (x - mean) / (std + norm_eps) of the
    evaluate scripts is applied in the same pass (avvad_stft_features)."""
    w, w2 = _wave2d(wave)
    B, Ls = w2.shape
    T = n_frames(Ls, n_fft, hop, pad_at_end, fs)
    F = n_fft // 2 + 1
    d = L.StftDesc(B, Ls, n_fft, hop, T, float(eps))
    ws = _ws(L.lib().avvad_stft_workspace(C.byref(d)), w.device)
    out = torch.empty((F, T, 2) if mode == 2 else (B, T, F), dtype=torch.float32, device=w.device)
    if mean is not None:
        if mode != 0 or std is None:
            raise L.AvvadError("standardisation is fused into the log-power mode only and needs both mean and std")
        mean, std = _mean_std(mean, std, F)
        L.check(L.lib().avvad_stft_features(L.ptr(w2), L.ptr(mean), L.ptr(std), L.ptr(out), C.byref(d), float(norm_eps), L.ptr(ws),
                                            ws.numel() * 4, _stream()), "avvad_stft_features")
        return out
    L.check(L.lib().avvad_stft(L.ptr(w2), L.ptr(out), C.byref(d), mode, L.ptr(ws), ws.numel() * 4, _stream()), "avvad_stft")
    return out


def peak_normalize(wave):
    """x / max|x| per utterance (evaluate_audio_net.py:125-127); wave (B,L) or (L,)."""
    w, w2 = _wave2d(wave)
    out = torch.empty_like(w2)
    L.check(L.lib().avvad_peak_normalize(L.ptr(w2), L.ptr(out), w2.shape[0], w2.shape[1], _stream()), "avvad_peak_normalize")
    return out.view(w.shape)


def standardize(x, mean, std, eps=1e-8):
    """(x - mean.T) / (std + eps).T of the train / evaluate loops (train_AV_net.py:286-291).  ``mean`` / ``std`` hold
    either one value per feature of the last axis (audio: (513,1)) or a single value (video: (1,1))."""
    x = _dev(x, "x")
    mean, std = _dev(mean, "mean").reshape(-1), _dev(std, "std").reshape(-1)
    F = x.shape[-1]
    nstat = mean.numel()
    if std.numel() != nstat or nstat not in (1, F):
        raise L.AvvadError("standardize: statistics must hold 1 or %d values, got %d / %d" % (F, nstat, std.numel()))
    out = torch.empty_like(x)
    L.check(L.lib().avvad_standardize(L.ptr(x), L.ptr(mean), L.ptr(std), L.ptr(out), x.numel() // F, F, nstat, float(eps),
                                      _stream()), "avvad_standardize")
    return out


# --------------------------------------------------------------------------- masked inverse STFT (csrc/istft.hip)
def istft_length(T, n_fft, hop, center=False):
    """Samples librosa's ``istft`` returns for T frames when no ``length`` is given: ``n_fft + hop (T - 1)``, less
    ``n_fft/2`` at either end when ``center``."""
    T, n_fft, hop = int(T), int(n_fft), int(hop)
    if T < 1:
        return 0
    return n_fft + hop * (T - 1) - (2 * (n_fft // 2) if center else 0)


def stft_complex(wave, n_fft=1024, hop=256, pad_at_end=True, fs=16e3):
    """wave (B,L) or (L,) on the GPU -> the complex spectrum of ``stft``'s DFT as a real (B,T,F,2) tensor (re, im)."""
    w, w2 = _wave2d(wave)
    B, Ls = w2.shape
    T = n_frames(Ls, n_fft, hop, pad_at_end, fs)
    d = L.StftDesc(B, Ls, n_fft, hop, T, 0.0)
    ws = _ws(L.lib().avvad_stft_workspace(C.byref(d)), w.device)
    out = torch.empty((B, T, n_fft // 2 + 1, 2), dtype=torch.float32, device=w.device)
    L.check(L.lib().avvad_stft_complex(L.ptr(w2), L.ptr(out), C.byref(d), L.ptr(ws), ws.numel() * 4, _stream()), "avvad_stft_complex")
    return out


def _mask_args(mask, mask_mode, B, T, F):
    if mask_mode is None:
        mask_mode = 0 if mask is None else 1
    mask_mode = int(mask_mode)
    if mask_mode not in (0, 1, 2, 3):
        raise L.AvvadError("mask_mode must be 0 (none), 1 (mask), 2 (sigmoid of logits) or 3 (logits > 0), got %r" % (mask_mode,))
    if mask_mode == 0:
        if mask is not None:
            raise L.AvvadError("mask_mode 0 takes no mask")
        return None, 0
    m = _dev(mask, "mask")
    if m.numel() != B * T * F or m.shape[-1] != F:
        raise L.AvvadError("mask must be (%d, %d, %d), got shape %s" % (B, T, F, tuple(m.shape)))
    return m, mask_mode


def _row_counts(v, B, hi, name, device):
    """per-row int32 counts on the device (None stays None) and the host list"""
    if v is None:
        return None, None
    vals = _ints(v, B, hi, "%s must hold %d values within 0..%d" % (name, B, hi))
    return torch.tensor(vals, dtype=torch.int32).to(device), vals


class MaskedInverseFn(torch.autograd.Function):
    """The graph node of ``istft`` / ``resynth`` for a mask (mode 1) or its logits (mode 2) that require a gradient.
    ``fwd(mask)`` is the very call the graph-less path makes, so the output keeps its bits; ``bwd(mask, dout)`` calls the
    ``_bwd`` entry point.  The spectrum / waveform is data: no gradient for it, and no double backward."""

    @staticmethod
    def forward(ctx, mask, fwd, bwd):
        ctx.bwd = bwd
        ctx.save_for_backward(mask)
        return fwd(mask)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        (mask,) = ctx.saved_tensors
        return ctx.bwd(mask, _dev(dout, "dout")).view(mask.shape), None, None


def _masked_inverse(mask, mode, fwd, bwd):
    """``fwd(mask)``, with a graph when the mask asks for one (modes 1 and 2 only: 0 has no mask, 3 no derivative)"""
    if mode in (1, 2) and mask.requires_grad and torch.is_grad_enabled():
        return MaskedInverseFn.apply(mask, fwd, bwd)
    return fwd(mask)


def istft(spec, n_fft=1024, hop=256, mask=None, mask_mode=None, n_frames=None, length=None, center=False, scale=None):
    """Masked inverse STFT on the GPU (librosa's ``istft``: Hann synthesis window, overlap-add, window sum-of-squares
    normalisation).  ``spec``: (B,T,F,2) (re, im), or ONE utterance in the legacy (F,T,2) layout ``stft_pytorch`` returns,
    or a complex64 (F,T) tensor; read in place through its strides.  ``mask`` (B,T,F) with ``mask_mode`` 1 (multiply;
    the default when a mask is given), 2 (``sigmoid(mask)``) or 3 (``mask > 0``); the product is formed while the spectrum
    is loaded.  ``n_frames``: frames per row (default T); ``length``: output samples, one value or one per row (default
    ``istft_length`` of the row's frames); ``center`` trims ``n_fft/2`` at the start; ``scale`` (B,) multiplies each row.
    Returns (B, Lout); samples past a row's length are zero.  A mask (mode 1) or logits (mode 2) that require a gradient
    get one (avvad_istft_bwd); the spectrum is data and gets none."""
    legacy = False
    if isinstance(spec, torch.Tensor) and spec.is_complex():
        if spec.dtype != torch.complex64 or spec.dim() != 2:
            raise L.AvvadError("a complex spectrum must be a complex64 (F, T) tensor, got %s %s" % (spec.dtype, tuple(spec.shape)))
        spec = torch.view_as_real(spec)
    if not isinstance(spec, torch.Tensor) or not spec.is_cuda:
        raise L.AvvadError("spec must be a GPU tensor: the inverse STFT has no CPU fallback")
    if spec.dtype != torch.float32 or spec.dim() not in (3, 4) or spec.shape[-1] != 2:
        raise L.AvvadError("spec must be float32 (B,T,F,2) or (F,T,2), or complex64 (F,T); got %s %s" % (spec.dtype, tuple(spec.shape)))
    n_fft, hop = int(n_fft), int(hop)
    F = n_fft // 2 + 1
    if spec.dim() == 3:
        legacy = True
        if spec.stride(2) != 1 or spec.stride(0) <= 0 or spec.stride(1) <= 0:
            spec = spec.contiguous()
        B, T = 1, spec.shape[1]
        strides = (0, spec.stride(1), spec.stride(0))
    else:
        spec = spec.contiguous()
        B, T = spec.shape[0], spec.shape[1]
        strides = (T * F * 2, F * 2, 2)
    if spec.shape[0 if legacy else 2] != F:
        raise L.AvvadError("spec holds %d bins, n_fft = %d has %d" % (spec.shape[0 if legacy else 2], n_fft, F))
    if T < 1:
        raise L.AvvadError("spec holds no frame")
    m, mode = _mask_args(mask, mask_mode, B, T, F)
    nf_dev, nf = _row_counts(n_frames, B, T, "n_frames", spec.device)
    if length is None:
        lens = [istft_length(n, n_fft, hop, center) for n in (nf if nf is not None else [T] * B)]
    elif isinstance(length, (list, tuple, torch.Tensor)):
        lens = _ints(length, B, None, "length must hold %d non-negative values" % B)
    else:
        lens = [int(length)] * B
    Lout = max(lens)
    if Lout < 1:
        raise L.AvvadError("the output would be empty (length %r, %d frames)" % (length, T))
    len_dev = None if min(lens) == Lout else torch.tensor(lens, dtype=torch.int32).to(spec.device)
    sc = None if scale is None else _row_vector(scale, B, "scale")
    d = L.IstftDesc(B, T, n_fft, hop, n_fft // 2 if center else 0, Lout, mode)

    def fwd(m):
        m = None if m is None else m.detach()
        out = torch.empty(B, Lout, dtype=torch.float32, device=spec.device)
        with torch.cuda.device(spec.device):
            ws = _ws(L.lib().avvad_istft_workspace(C.byref(d)), spec.device)
            L.check(L.lib().avvad_istft(L.ptr(spec), strides[0], strides[1], strides[2], L.ptr(m), L.ptr(nf_dev), L.ptr(len_dev),
                                        L.ptr(sc), L.ptr(out), C.byref(d), L.ptr(ws), ws.numel() * 4, _stream()), "avvad_istft")
        return out

    def bwd(m, dout):
        dmask = torch.empty(B, T, F, dtype=torch.float32, device=spec.device)
        with torch.cuda.device(spec.device):
            ws = _ws(L.lib().avvad_istft_bwd_workspace(C.byref(d)), spec.device)
            L.check(L.lib().avvad_istft_bwd(L.ptr(spec), strides[0], strides[1], strides[2], L.ptr(m), L.ptr(nf_dev), L.ptr(len_dev),
                                            L.ptr(sc), L.ptr(dout), L.ptr(dmask), C.byref(d), L.ptr(ws), ws.numel() * 4, _stream()),
                    "avvad_istft_bwd")
        return dmask
    return _masked_inverse(m, mode, fwd, bwd)


def resynth(wave, mask, mask_mode=1, n_fft=1024, hop=256, sample_lengths=None, pad_at_end=True, fs=16e3, scale=None):
    """mask x STFT(wave) -> waveform in one call (avvad_resynth): the forward DFT of ``stft``, the masked inverse and the
    overlap-add, the spectrum never leaving the workspace.  wave (B,L) zero-padded rows (or (L,)), ``sample_lengths`` the
    B real lengths (default L); ``mask`` (B,T,F) with T = ``n_frames(L)``, read by ``mask_mode`` as in ``istft`` (``None``
    with mode 0).  Row b uses its own ``n_frames(L_b)`` frames and comes back with exactly L_b samples, zero behind them
    (cropped where the frames run past the utterance -- the end pad -- and zero-filled where they stop short of it).
    Returns (B, L).  A mask (mode 1) or logits (mode 2) that require a gradient get one (avvad_resynth_bwd, which
    transforms the wave again); the wave is data and gets none."""
    w, w2 = _wave2d(wave)
    B, Ls = w2.shape
    n_fft, hop = int(n_fft), int(hop)
    T = n_frames(Ls, n_fft, hop, pad_at_end, fs)
    if T < 1:
        raise L.AvvadError("a wave of %d samples holds no %d-sample frame" % (Ls, n_fft))
    F = n_fft // 2 + 1
    m, mode = _mask_args(mask, mask_mode, B, T, F)
    len_dev, lens = _row_counts(sample_lengths, B, Ls, "sample_lengths", w.device)
    nf_dev = None
    if lens is not None:
        nf_dev = torch.tensor([min(T, max(0, n_frames(n, n_fft, hop, pad_at_end, fs))) for n in lens], dtype=torch.int32).to(w.device)
    sc = None if scale is None else _row_vector(scale, B, "scale")
    sd = L.StftDesc(B, Ls, n_fft, hop, T, 0.0)
    d = L.IstftDesc(B, T, n_fft, hop, 0, Ls, mode)

    def fwd(m):
        m = None if m is None else m.detach()
        ws = _ws(L.lib().avvad_resynth_workspace(C.byref(sd), C.byref(d)), w.device)
        out = torch.empty(B, Ls, dtype=torch.float32, device=w.device)
        L.check(L.lib().avvad_resynth(L.ptr(w2), L.ptr(m), L.ptr(nf_dev), L.ptr(len_dev), L.ptr(sc), L.ptr(out), C.byref(sd),
                                      C.byref(d), L.ptr(ws), ws.numel() * 4, _stream()), "avvad_resynth")
        return out

    def bwd(m, dout):
        ws = _ws(L.lib().avvad_resynth_bwd_workspace(C.byref(sd), C.byref(d)), w.device)
        dmask = torch.empty(B, T, F, dtype=torch.float32, device=w.device)
        L.check(L.lib().avvad_resynth_bwd(L.ptr(w2), L.ptr(m), L.ptr(nf_dev), L.ptr(len_dev), L.ptr(sc), L.ptr(dout), L.ptr(dmask),
                                          C.byref(sd), C.byref(d), L.ptr(ws), ws.numel() * 4, _stream()), "avvad_resynth_bwd")
        return dmask
    return _masked_inverse(m, mode, fwd, bwd)


# --------------------------------------------------------------------------- streaming STFT front-end (csrc/stft_stream.hip)
def _n_fft_check(n_fft):
    n_fft = int(n_fft)
    if n_fft < 32 or n_fft % 32 or n_fft > 2048:
        raise L.AvvadError("the streaming front-end needs 32 <= n_fft <= 2048 and n_fft %% 32 == 0, got %d" % n_fft)
    return n_fft


def peak(wave):
    """max|x| per utterance, (B,): the constant ``peak_normalize`` divides by; wave (B,L) or (L,)."""
    w, w2 = _wave2d(wave)
    out = torch.empty(w2.shape[0], dtype=torch.float32, device=w.device)
    L.check(L.lib().avvad_abs_max(L.ptr(w2), L.ptr(out), w2.shape[0], w2.shape[1], _stream()), "avvad_abs_max")
    return out


def _stream_basis(which, n_fft, device):
    """the packed basis of ``avvad_<which>_basis``, sized by ``avvad_<which>_basis_bytes``"""
    n_fft = _n_fft_check(n_fft)
    out = torch.empty(getattr(L.lib(), "avvad_%s_basis_bytes" % which)(n_fft) // 4, dtype=torch.float32, device=device)
    if not out.is_cuda:
        raise L.AvvadError("the basis lives on the GPU: no CPU fallback")
    with torch.cuda.device(out.device):
        L.check(getattr(L.lib(), "avvad_%s_basis" % which)(n_fft, L.ptr(out), _stream()), "avvad_%s_basis" % which)
    return out


def _stream_state(B, width, device):
    """zeroed per-row state (B, width) of a streaming stage"""
    if int(B) < 1:
        raise L.AvvadError("B must be >= 1")
    return torch.zeros(int(B), width, dtype=torch.float32, device=device)


def _stream_chunk(chunk, n_valid):
    """The samples of a streaming call -> (chunk (B, n), B, n, the real samples per row (``n_valid`` None: all n))."""
    chunk = _dev(chunk, "chunk")
    if chunk.dim() != 2 or chunk.shape[0] < 1:
        raise L.AvvadError("chunk must be (B, n) samples, got %s" % (tuple(chunk.shape),))
    B, n = chunk.shape
    return chunk, B, n, _ints(n_valid, B, n, default=n, what="n_valid")


def _stream_buffers(state, out_state, shape, device, made_by, *args):
    """Checks ``state`` / ``out_state`` of a streaming stage against the ``shape`` of ``made_by % args`` (the ``*_state(...)``
    call the message quotes).  -> (in_place, the tensor the kernel writes the new state to): with ``out_state`` None or
    ``state`` itself a temporary, which ``_stream_commit`` copies back into ``state`` after the launch."""
    def st(t, what):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or \
                tuple(t.shape) != shape or t.device != device:
            raise L.AvvadError("%s must be the contiguous float32 GPU tensor of %s" % (what, made_by % args))
    st(state, "state")
    if out_state is not None and out_state is not state:
        st(out_state, "out_state")
    in_place = out_state is None or out_state.data_ptr() == state.data_ptr()
    return in_place, torch.empty_like(state) if in_place else out_state


def _stream_commit(in_place, state, new):
    if in_place:
        state.copy_(new)


def _stream_table(t, what, dtype, numel, device, made_by, *args):
    """Checks a table built once per stream (a packed basis, the resampler's taps): dtype, device and size."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or t.device != device or \
            not t.is_contiguous() or t.numel() != numel:
        raise L.AvvadError("%s must be %s" % (what, made_by % args))


def stft_stream_basis(n_fft, device):
    """The windowed DFT basis of ``stft`` in the streaming kernel's packed layout (an opaque float tensor): built once,
    reused by every ``stft_stream`` call with that ``n_fft``."""
    return _stream_basis("stft_stream", n_fft, device)


def stft_stream_state(B, n_fft, device):
    """Zeroed front-end state (B, n_fft) -- each row's pending samples; all zeros with a count of 0 (a fresh
    ``SampleClock``) is "start of utterance"."""
    return _stream_state(B, _n_fft_check(n_fft), device)


def _row_vector(v, B, name):
    v = _dev(v, name).reshape(-1)
    if v.numel() != B:
        raise L.AvvadError("%s must hold one value per row (%d), got %d" % (name, B, v.numel()))
    return v


def stft_stream(chunk, n_valid, clock, state, basis, peak=None, mean=None, std=None, final=None, out_state=None, eps=1e-8,
                norm_eps=1e-8, return_spec=False):
    """The next samples of ``B`` rows through the STFT front-end (inference only): one kernel launch.

    chunk (B, n) float32 on the GPU, of which row b's first ``n_valid[b]`` samples are real (None: all n).  ``clock``
    is the rows' :class:`avvad.stream.SampleClock` (n_fft, hop and the per-row counts); it is advanced by this call.
    ``state`` (B, n_fft) from ``stft_stream_state`` holds the pending samples; the new tails go to ``out_state`` -- a spare
    tensor the caller swaps with ``state`` -- or, with ``out_state`` None or ``state`` itself, back into ``state``.
    ``peak`` (B,): every sample is divided by its row's value (None: 1, which changes no bit).  ``mean`` / ``std`` (F each):
    the standardisation of ``stft(mean=, std=)``.  ``final``: rows that end with this call; they also yield the
    reference's zero-padded last frame where it has one and must be reset on the clock before they take samples again.
    -> (features (B, tmax, F) with tmax = max(frames) and zeros behind a row's frames, frames per row (list)).
    ``return_spec``: -> (features, frames, spec (B, tmax, F, 2)), the complex spectrum (re, im) of the samples / peak that
    the same launch holds anyway (zeros behind a row's frames); the features keep their bits.  What ``istft_stream`` takes.
    Every argument is checked before the clock or a state changes.  Any split of a stream into calls gives the same bits."""
    chunk, B, n, nv = _stream_chunk(chunk, n_valid)
    n_fft, hop = _n_fft_check(clock.n_fft), int(clock.hop)
    F = n_fft // 2 + 1
    in_place, new = _stream_buffers(state, out_state, (B, n_fft), chunk.device, "stft_stream_state(%d, %d, device)", B, n_fft)
    _stream_table(basis, "basis", torch.float32, L.lib().avvad_stft_stream_basis_bytes(n_fft) // 4, chunk.device,
                  "stft_stream_basis(%d, device)", n_fft)
    pk = None if peak is None else _row_vector(peak, B, "peak")
    if (mean is None) != (std is None):
        raise L.AvvadError("standardisation needs both mean and std")
    if mean is not None:
        mean, std = _mean_std(mean, std, F)
    frames, pending, pad = clock.advance(nv, final=() if final is None else final)      # raises before it changes anything
    tmax = max(frames)
    counts = torch.tensor([nv, pending, frames, pad], dtype=torch.int32).to(chunk.device, non_blocking=False)
    out = torch.empty(B, tmax, F, dtype=torch.float32, device=chunk.device)
    src = chunk if n > 0 else chunk.new_zeros(B, 1)
    d = L.StftStreamDesc(B, max(n, 1), n_fft, hop, tmax, sum(frames), float(eps), float(norm_eps))
    spec = torch.empty(B, tmax, F, 2, dtype=torch.float32, device=chunk.device) if return_spec else None
    with torch.cuda.device(chunk.device):
        args = (L.ptr(src), L.ptr(counts[0]), L.ptr(counts[1]), L.ptr(counts[2]), L.ptr(counts[3]), L.ptr(pk), L.ptr(state),
                L.ptr(new), L.ptr(basis), L.ptr(mean), L.ptr(std), L.ptr(out) if tmax else None)
        if return_spec:
            L.check(L.lib().avvad_stft_stream_fwd_spec(*args, L.ptr(spec) if tmax else None, C.byref(d), _stream()),
                    "avvad_stft_stream_fwd_spec")
        else:
            L.check(L.lib().avvad_stft_stream_fwd(*args, C.byref(d), _stream()), "avvad_stft_stream_fwd")
    _stream_commit(in_place, state, new)
    return (out, frames, spec) if return_spec else (out, frames)


# --------------------------------------------------------------------------- streaming masked inverse (csrc/istft_stream.hip)
def istft_stream_basis(n_fft, device):
    """The windowed inverse-DFT basis of ``istft`` in the streaming kernel's packed layout, with the squared window behind
    it (an opaque float tensor): built once, reused by every ``istft_stream`` call with that ``n_fft``."""
    return _stream_basis("istft_stream", n_fft, device)


def istft_stream_state(B, n_fft, device):
    """Zeroed overlap-add state (B, n_fft) -- each row's unfinished sums of the samples later frames still cover; all
    zeros (a fresh ``OlaClock``) is "start of utterance"."""
    return _stream_state(B, _n_fft_check(n_fft), device)


def istft_stream(spec, frames, clock, state, basis, mask=None, mask_mode=None, scale=None, final_samples=None, out_state=None):
    """The next frames of ``B`` rows through the masked inverse STFT (inference only): the samples no later frame can
    cover any more, at a cost that does not depend on the position in the stream.

    spec (B, T, F, 2) float32 on the GPU as ``stft_stream(return_spec=True)`` returns it, of which row b's first
    ``frames[b]`` frames are real; ``mask`` (B, T, F) with ``mask_mode`` as in ``istft`` (modes 2 and 3 take logits).
    ``clock`` is the rows' :class:`avvad.stream.OlaClock` (n_fft, hop and the per-row counts); it is advanced by this call.
    ``state`` (B, n_fft) from ``istft_stream_state``; the new sums go to ``out_state`` -- a spare tensor the caller swaps
    with ``state`` -- or, with ``out_state`` None or ``state`` itself, back into ``state``.  ``scale`` (B,) multiplies each
    row (the peak the forward divided by).  ``final_samples``: {row: N} (or a list with None for rows that go on) -- the
    row's stream ends with this call and held N samples: it returns what is left of them, cropped or zero-filled like
    ``resynth``'s rows, and must be reset on the clock before it takes frames again.
    A row that goes on returns ``frames[b] * hop`` samples: a sample comes out up to ``n_fft - 1`` samples after it went in.
    -> (samples (B, nmax) with zeros behind a row's count, samples per row (list)).
    Every argument is checked before the clock or a state changes.  Any split of a stream into calls gives the same bits."""
    if not isinstance(spec, torch.Tensor) or not spec.is_cuda:
        raise L.AvvadError("spec must be a GPU tensor: the streaming inverse STFT has no CPU fallback")
    n_fft, hop = _n_fft_check(clock.n_fft), int(clock.hop)
    F = n_fft // 2 + 1
    if spec.dtype != torch.float32 or spec.dim() != 4 or spec.shape[0] < 1 or tuple(spec.shape[2:]) != (F, 2):
        raise L.AvvadError("spec must be float32 (B, T, %d, 2), got %s %s" % (F, spec.dtype, tuple(spec.shape)))
    spec = spec.contiguous()
    B, T = spec.shape[0], spec.shape[1]
    nf = _ints(frames, B, T, "frames must hold %d counts within 0..%d" % (B, T))
    if T > 0:
        m, mode = _mask_args(mask, mask_mode, B, T, F)
    else:
        m, mode = None, 0                                         # no row has a frame: there is nothing to mask
    in_place, new = _stream_buffers(state, out_state, (B, n_fft), spec.device, "istft_stream_state(%d, %d, device)", B, n_fft)
    _stream_table(basis, "basis", torch.float32, L.lib().avvad_istft_stream_basis_bytes(n_fft) // 4, spec.device,
                  "istft_stream_basis(%d, device)", n_fft)
    sc = None if scale is None else _row_vector(scale, B, "scale")
    n_before, n_out = clock.advance(nf, final_samples)           # raises before it changes anything
    nmax = max(n_out)
    counts = torch.tensor([nf, n_before, n_out], dtype=torch.int32).to(spec.device, non_blocking=False)
    out = torch.empty(B, nmax, dtype=torch.float32, device=spec.device)
    d = L.IstftStreamDesc(B, T, n_fft, hop, nmax, sum(nf), mode)
    with torch.cuda.device(spec.device):
        ws = _ws(L.lib().avvad_istft_stream_workspace(C.byref(d)), spec.device)
        L.check(L.lib().avvad_istft_stream(L.ptr(spec) if T else None, L.ptr(m), L.ptr(counts[0]), L.ptr(counts[1]),
                                           L.ptr(counts[2]), L.ptr(sc), L.ptr(state), L.ptr(new), L.ptr(basis),
                                           L.ptr(out) if nmax else None, C.byref(d), L.ptr(ws), ws.numel() * 4, _stream()),
                "avvad_istft_stream")
    _stream_commit(in_place, state, new)
    return out, n_out


# --------------------------------------------------------------------------- resampling (csrc/resample.hip)
_RESAMPLE_TAPS = {}


def resample_ratio(fs_in, fs_out=16000):
    """(up, down) of the rates ``fs_in -> fs_out`` in lowest terms; integer rates >= 1 whose reduced ratio stays within
    ``AVVAD_RESAMPLE_MAX_RATE``."""
    if any(isinstance(f, bool) or int(f) != f or int(f) < 1 for f in (fs_in, fs_out)):
        raise L.AvvadError("resample: rates must be integers >= 1, got %r -> %r" % (fs_in, fs_out))
    fs_in, fs_out = int(fs_in), int(fs_out)
    g = math.gcd(fs_in, fs_out)
    up, down = fs_out // g, fs_in // g
    if max(up, down) > L.RESAMPLE_MAX_RATE:
        raise L.AvvadError("resample: %d -> %d Hz is the ratio %d/%d, beyond %d" % (fs_in, fs_out, up, down, L.RESAMPLE_MAX_RATE))
    return up, down


def _ratio_check(up, down):
    if isinstance(up, bool) or isinstance(down, bool) or int(up) != up or int(down) != down:
        raise L.AvvadError("resample: up and down must be integers, got %r/%r" % (up, down))
    up, down = int(up), int(down)
    if up < 1 or down < 1 or max(up, down) > L.RESAMPLE_MAX_RATE or math.gcd(up, down) != 1 or up == down:
        raise L.AvvadError("resample: the ratio must be in lowest terms within 1..%d and not 1/1, got %d/%d"
                           % (L.RESAMPLE_MAX_RATE, up, down))
    return up, down


def resample_taps(up, down):
    """The resampler's host table: the ``2 * half + 1`` float64 taps (``half = 10 * max(up, down)``)
    ``up * firwin(2 * half + 1, 1 / max(up, down), window=('kaiser', 5.0))`` that ``scipy.signal.resample_poly(x, up, down)``
    uses by default, built with numpy alone (windowed sinc, DC gain 1, times ``up``).  ``resample_taps(5, 8)`` is
    ``stoi_taps()`` bit for bit."""
    import numpy as np
    up, down = _ratio_check(up, down)
    m = max(up, down)
    half = 10 * m
    fc = 1.0 / m
    k = np.arange(2 * half + 1, dtype=np.float64) - float(half)
    h = fc * np.sinc(fc * k) * np.kaiser(2 * half + 1, 5.0)
    return float(up) * (h / h.sum())


def resample_taps_phase_major(up, down):
    """``resample_taps`` in the kernel's layout (include/avvad.h): ``T = 2 * half // up + 1`` taps per phase,
    ``taps[p * T + j] = h[p + j * up]`` and 0 behind the last tap."""
    import numpy as np
    h = resample_taps(up, down)
    up = int(up)
    T = (len(h) - 1) // up + 1
    tp = np.zeros((up, T), dtype=np.float64)
    for p in range(up):
        col = h[p::up]
        tp[p, :len(col)] = col
    return tp.reshape(-1)


def resample_taps_on(up, down, device):
    """The phase-major taps of a ratio on ``device``: built once per (ratio, device), what ``resample_stream`` takes."""
    up, down = _ratio_check(up, down)
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (up, down, device)
    taps = _RESAMPLE_TAPS.get(key)
    if taps is None:
        taps = _RESAMPLE_TAPS[key] = torch.from_numpy(resample_taps_phase_major(up, down)).to(device)
    return taps


def resample_length(n, up, down):
    """Samples ``n`` inputs give: ``ceil(n * up / down)``."""
    up, down = _ratio_check(up, down)
    if int(n) < 0:
        raise L.AvvadError("resample_length: negative sample count %r" % (n,))
    return (int(n) * up + down - 1) // down


def resample(wave, lengths=None, fs_in=None, fs_out=16000):
    """A ragged batch from ``fs_in`` to ``fs_out`` on the GPU (avvad_resample), with ``scipy.signal.resample_poly``'s default
    filter: wave (B, L) (or (L,)) float32, row b's first ``lengths[b]`` samples real (nothing behind them is read; None: all).
    -> (out (B, Lout) -- (Lout,) for a 1-D wave -- with ``Lout = resample_length(L)`` and zeros behind a row's samples,
    samples per row (list)).  ``fs_in == fs_out`` returns the input itself.  Every sample is a double sum in a fixed order
    rounded once: the same bits from run to run, at any batch, and as ``resample_stream`` gives for any split."""
    if fs_in is None:
        raise L.AvvadError("resample: fs_in is required")
    up, down = resample_ratio(fs_in, fs_out)
    if not isinstance(wave, torch.Tensor) or wave.dim() not in (1, 2) or (wave.numel() == 0 and up != down):
        raise L.AvvadError("resample: wave must be a GPU tensor (B, L) or (L,) with L >= 1, got %s"
                           % (tuple(getattr(wave, "shape", ())),))
    B, Ls = (1, wave.shape[0]) if wave.dim() == 1 else wave.shape
    lens = [Ls] * B if lengths is None else _ints(lengths, B, Ls, "lengths must hold %d values within 0..%d" % (B, Ls))
    if up == down:
        return wave, lens
    x, ld_x = _score_rows(wave, "wave", B, Ls)
    lens32 = None if lengths is None else torch.tensor(lens, dtype=torch.int32).to(x.device)
    taps = resample_taps_on(up, down, x.device)
    Lout = resample_length(Ls, up, down)
    out = torch.empty(B, Lout, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        L.check(L.lib().avvad_resample(L.ptr(x), ld_x, L.ptr(lens32), L.ptr(taps), up, down, L.ptr(out), Lout, None, B, Ls,
                                       _stream()), "avvad_resample")
    return (out[0] if wave.dim() == 1 else out), [resample_length(n, up, down) for n in lens]


def resample_stream_state(B, up, down, device):
    """Zeroed resampler state (B, H), ``H = 2 * half // up + 2``: the last inputs of each row, which later outputs still
    need; with a fresh ``RateClock`` it is "start of utterance" whatever it holds."""
    return _stream_state(B, L.lib().avvad_resample_hist(*_ratio_check(up, down)), device)


def resample_stream(chunk, n_valid, clock, state, taps, final=None, out_state=None):
    """The next samples of ``B`` rows through the resampler (avvad_resample_stream): one kernel launch.

    chunk (B, n) float32 on the GPU at the input rate, of which row b's first ``n_valid[b]`` samples are real (None: all n).
    ``clock`` is the rows' :class:`avvad.stream.RateClock` (the ratio and the per-row counts); it is advanced by this call.
    ``state`` (B, H) from ``resample_stream_state``; the new tails go to ``out_state`` -- a spare tensor the caller swaps with
    ``state`` -- or, with ``out_state`` None or ``state`` itself, back into ``state``.  ``taps``: ``resample_taps_on`` of the
    clock's ratio.  ``final``: rows that end with this call; they also yield the outputs whose later taps never came and
    must be reset on the clock before they take samples again.
    -> (out (B, nmax) with zeros behind a row's count, samples per row (list)).  A row that goes on has emitted
    ``floor((N * up - 1 - half) / down) + 1`` samples after N inputs; a stream of N samples yields exactly ``resample``'s.
    Every argument is checked before the clock or a state changes.  Any split of a stream into calls gives the same bits."""
    chunk, B, n, nv = _stream_chunk(chunk, n_valid)
    up, down = _ratio_check(clock.up, clock.down)
    in_place, new = _stream_buffers(state, out_state, (B, L.lib().avvad_resample_hist(up, down)), chunk.device,
                                    "resample_stream_state(%d, %d, %d, device)", B, up, down)
    _stream_table(taps, "taps", torch.float64, L.lib().avvad_resample_taps_len(up, down), chunk.device,
                  "resample_taps_on(%d, %d, device)", up, down)
    in_before, out_before, n_emit = clock.advance(nv, final=() if final is None else final)   # raises before it changes anything
    nmax = max(n_emit)
    counts = torch.tensor([nv, in_before, out_before, n_emit], dtype=torch.int64).to(chunk.device, non_blocking=False)
    out = torch.empty(B, nmax, dtype=torch.float32, device=chunk.device)
    with torch.cuda.device(chunk.device):
        L.check(L.lib().avvad_resample_stream(L.ptr(chunk) if n else None, n, L.ptr(counts[0]), L.ptr(counts[1]), L.ptr(counts[2]),
                                              L.ptr(counts[3]), L.ptr(state), L.ptr(new), L.ptr(taps), up, down,
                                              L.ptr(out) if nmax else None, nmax, B, n, nmax, _stream()), "avvad_resample_stream")
    _stream_commit(in_place, state, new)
    return out, n_emit


# --------------------------------------------------------------------------- train-set statistics (no gradient)
def stats_new(nstat, device):
    """A zeroed statistics accumulator: float64 ``[sum (nstat), sumsq (nstat), count]`` on the GPU (include/avvad.h,
    avvad_stats_*).  ``nstat`` is the feature width (per-bin statistics: audio, 513) or 1 (one scalar pair: video)."""
    if int(nstat) < 1:
        raise L.AvvadError("nstat must be positive, got %r" % (nstat,))
    if torch.device(device).type != "cuda":
        raise L.AvvadError("the statistics accumulate on the GPU: the AV-VAD hot path has no CPU fallback")
    return torch.zeros(2 * int(nstat) + 1, dtype=torch.float64, device=device)


def _acc_nstat(acc):
    if not isinstance(acc, torch.Tensor) or not acc.is_cuda or acc.dtype != torch.float64 or acc.dim() != 1 \
            or not acc.is_contiguous() or acc.numel() < 3 or acc.numel() % 2 == 0:
        raise L.AvvadError("acc must be a contiguous float64 GPU vector of 2 * nstat + 1 values (ops.stats_new)")
    return (acc.numel() - 1) // 2


def stft_stats(acc, wave, sample_lengths, n_fft=1024, hop=256, eps=1e-8, pad_at_end=True, fs=16e3):
    """Adds the log-power STFT features of a ragged batch to ``acc`` without writing them (avvad_stft_stats): wave (B, L)
    zero-padded rows (or (L,)), ``sample_lengths`` the B real lengths; row b counts its first ``n_frames(L_b)`` frames,
    the rule ``ops.stft`` uses for the frame count.  Returns ``acc``."""
    w, w2 = _wave2d(wave)
    B, Ls = w2.shape
    lens = _ints(sample_lengths, B, Ls, "sample_lengths must hold %d lengths within 0..%d" % (B, Ls))
    F = n_fft // 2 + 1
    if _acc_nstat(acc) != F:
        raise L.AvvadError("acc holds %d statistics, the STFT has %d bins" % (_acc_nstat(acc), F))
    T = n_frames(Ls, n_fft, hop, pad_at_end, fs)
    counts = torch.tensor([max(0, n_frames(n, n_fft, hop, pad_at_end, fs)) for n in lens], dtype=torch.int32).to(w.device)
    d = L.StftDesc(B, Ls, n_fft, hop, T, float(eps))
    ws = _ws(L.lib().avvad_stft_stats_workspace(C.byref(d)), w.device)
    L.check(L.lib().avvad_stft_stats(L.ptr(w2), L.ptr(counts), L.ptr(acc), C.byref(d), L.ptr(ws), ws.numel() * 4, _stream()),
            "avvad_stft_stats")
    return acc


def accumulate_stats(acc, x, lengths=None, nstat=None):
    """Adds materialised features x (B, T, F) (or (T, F)) to ``acc`` (avvad_stats_accumulate); rows t >= lengths[b] are
    not counted.  ``nstat`` (default: what ``acc`` holds) is F or 1 -- spectrogram batches of a loader, or video frames
    flattened to (B, T, H*W) with one scalar pair.  Returns ``acc``."""
    x = _dev(x, "x")
    if x.dim() == 2:
        x = x.view(1, *x.shape)
    if x.dim() != 3:
        raise L.AvvadError("x must be (B, T, F), got shape %s" % (tuple(x.shape),))
    B, T, F = x.shape
    have = _acc_nstat(acc)
    nstat = have if nstat is None else int(nstat)
    if nstat != have or nstat not in (1, F):
        raise L.AvvadError("accumulate_stats: statistics must hold 1 or %d values, acc holds %d, nstat %d" % (F, have, nstat))
    lens32 = None
    if lengths is not None:
        lens32 = lengths_i32(lengths, x.device)
        if lens32.numel() != B:
            raise L.AvvadError("lengths must hold %d values" % B)
    ws = _ws(L.lib().avvad_stats_workspace(B * T, nstat), x.device)
    L.check(L.lib().avvad_stats_accumulate(L.ptr(x), L.ptr(lens32), L.ptr(acc), B, T, F, nstat, L.ptr(ws), ws.numel() * 4,
                                           _stream()), "avvad_stats_accumulate")
    return acc


def finalize_stats(acc):
    """(mean, std) float32 (nstat,) on the GPU: ``mean = sum / n``, ``std = sqrt((sumsq - n mean^2) / (n - 1))`` in
    double (avvad_stats_finalize).  Fewer than two counted values raise."""
    nstat = _acc_nstat(acc)
    n = float(acc[-1])
    if not n >= 2:
        raise L.AvvadError("statistics of %g values: mean / empirical std need at least two" % n)
    mean = torch.empty(nstat, dtype=torch.float32, device=acc.device)
    std = torch.empty_like(mean)
    L.check(L.lib().avvad_stats_finalize(L.ptr(acc), nstat, L.ptr(mean), L.ptr(std), _stream()), "avvad_stats_finalize")
    return mean, std


# --------------------------------------------------------------------------- scores (no gradient)
SCORE_CHUNK = L.SCORE_CHUNK      # samples of one partial of the energy-ratio pass (include/avvad.h AVVAD_SCORE_CHUNK)
_THIRD = {None: 0, "none": 0, "noise": 1, "mixture": 2, 0: 0, 1: 1, 2: 2}


def score_state(B, device):
    """A zeroed score accumulator: float64 (B, 6) on the GPU, per row the inner products
    ``(e.e, e.r, e.n, r.r, n.n, r.n)`` of estimate, clean reference and noise (include/avvad.h, avvad_score_*)."""
    if int(B) < 1:
        raise L.AvvadError("B must be positive, got %r" % (B,))
    if torch.device(device).type != "cuda":
        raise L.AvvadError("the scores accumulate on the GPU: the AV-VAD hot path has no CPU fallback")
    return torch.zeros(int(B), 6, dtype=torch.float64, device=device)


def _score_acc(acc):
    if not isinstance(acc, torch.Tensor) or not acc.is_cuda or acc.dtype != torch.float64 or acc.dim() != 2 \
            or acc.shape[1] != 6 or not acc.is_contiguous():
        raise L.AvvadError("acc must be a contiguous float64 GPU tensor (B, 6) (ops.score_state)")
    return acc.shape[0]


def _score_rows(t, name, B, Ls):
    """(tensor to read in place, row pitch in floats) of a (B, >= Ls) or (>= Ls,) float32 GPU signal: read through its
    strides; only a last axis that is not unit-stride (or rows that overlap) is copied."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.AvvadError("%s must be a GPU tensor: the AV-VAD hot path has no CPU fallback" % name)
    if t.dtype != torch.float32:
        raise L.AvvadError("%s must be float32, got %s" % (name, t.dtype))
    if t.dim() == 1:
        t = t.view(1, -1)
    if t.dim() != 2 or t.shape[0] != B or t.shape[1] < Ls:
        raise L.AvvadError("%s must hold %d rows of at least %d samples, got shape %s" % (name, B, Ls, tuple(t.shape)))
    t = t[:, :Ls]
    if t.stride(1) != 1 or (B > 1 and t.stride(0) < Ls):
        t = t.contiguous()
    return t, (t.stride(0) if B > 1 else Ls)


def score_accumulate(acc, est, ref, noise=None, mixture=None, lengths=None):
    """Adds the inner products of a ragged batch to ``acc`` (avvad_score_accumulate): est (B, L) (or (L,)) the enhanced
    signal, ref the clean one, and as the third signal either ``noise`` or the noisy ``mixture`` (the kernel then forms
    ``noise = mixture - ref`` in double), or neither (SI-SDR alone).  ref / noise / mixture may have longer rows than est:
    their first L samples count.  Samples at or behind ``lengths[b]`` are not read.  Returns ``acc``."""
    B = _score_acc(acc)
    if noise is not None and mixture is not None:
        raise L.AvvadError("score_accumulate: give the noise or the mixture, not both")
    if not isinstance(est, torch.Tensor) or est.dim() not in (1, 2):
        raise L.AvvadError("est must be a (B, L) or (L,) GPU tensor")
    Ls = est.shape[-1]
    e, ld_e = _score_rows(est, "est", B, Ls)
    r, ld_r = _score_rows(ref, "ref", B, Ls)
    third, mode = (noise, 1) if noise is not None else (mixture, 2) if mixture is not None else (None, 0)
    t, ld_t = _score_rows(third, "noise" if mode == 1 else "mixture", B, Ls) if mode else (None, 0)
    lens32 = None
    if lengths is not None:
        lens32 = lengths_i32(lengths, e.device)
        if lens32.numel() != B:
            raise L.AvvadError("lengths must hold %d values" % B)
    ws = _ws(L.lib().avvad_score_workspace(B, Ls), e.device)
    L.check(L.lib().avvad_score_accumulate(L.ptr(e), ld_e, L.ptr(r), ld_r, L.ptr(t), ld_t, mode, L.ptr(lens32), L.ptr(acc), B, Ls,
                                           L.ptr(ws), ws.numel() * 4, _stream()), "avvad_score_accumulate")
    return acc


def score_finalize(acc, third, return_alpha=False):
    """(B, 3) float64 on the GPU: ``si_sdr, si_sir, si_sar`` in dB from a score accumulator (avvad_score_finalize).
    ``third``: what the accumulate calls were given -- "noise", "mixture" or "none" (None); with "none" only SI-SDR is
    defined and the other two are NaN.  An empty row is NaN.  ``return_alpha``: also (B, 2) ``alpha_s, alpha_n``."""
    B = _score_acc(acc)
    if third not in _THIRD:
        raise L.AvvadError("third must be 'none', 'noise' or 'mixture', got %r" % (third,))
    ratios = torch.empty((B, 3), dtype=torch.float64, device=acc.device)
    alpha = torch.empty((B, 2), dtype=torch.float64, device=acc.device) if return_alpha else None
    L.check(L.lib().avvad_score_finalize(L.ptr(acc), B, _THIRD[third], L.ptr(ratios), L.ptr(alpha), _stream()), "avvad_score_finalize")
    return (ratios, alpha) if return_alpha else ratios


def energy_ratios(est, ref, noise=None, mixture=None, lengths=None, return_alpha=False):
    """``packages/metrics.py energy_ratios`` of a ragged batch in one call: (B, 3) float64 ``si_sdr, si_sir, si_sar`` on
    the GPU (and (B, 2) ``alpha_s, alpha_n`` with ``return_alpha``).  Arguments as for ``score_accumulate``."""
    if not isinstance(est, torch.Tensor) or not est.is_cuda:
        raise L.AvvadError("est must be a GPU tensor: the AV-VAD hot path has no CPU fallback")
    acc = score_state(1 if est.dim() == 1 else est.shape[0], est.device)
    score_accumulate(acc, est, ref, noise, mixture, lengths)
    return score_finalize(acc, "noise" if noise is not None else "mixture" if mixture is not None else "none", return_alpha)


# --------------------------------------------------------------------------- STOI / ESTOI (csrc/stoi.hip, no gradient)
_STOI_TAPS = {}


def stoi_taps():
    """The resampler's host table: the 161 float64 taps ``5 * firwin(161, 1/8, window=('kaiser', 5.0))`` that
    ``scipy.signal.resample_poly(x, 5, 8)`` uses by default, built with numpy alone (windowed sinc, DC gain 1, times 5)."""
    import numpy as np
    m = np.arange(161, dtype=np.float64) - 80.0
    h = 0.125 * np.sinc(0.125 * m) * np.kaiser(161, 5.0)
    return 5.0 * (h / h.sum())


def _stoi_taps_on(device):
    taps = _STOI_TAPS.get(device)
    if taps is None:
        taps = _STOI_TAPS[device] = torch.from_numpy(stoi_taps()).to(device)
    return taps


def stoi(clean, processed, lengths=None, fs=16000, extended=False, both=False, return_info=False):
    """STOI (``extended``: ESTOI) of a ragged batch on the GPU (avvad_stoi): clean and processed (B, L) (or (L,)) float32,
    cropped to ``lengths`` (nothing at or behind a row's length is read).  ``fs`` 16000 (resampled to 10 kHz) or 10000.
    Returns float64 (B,) on the GPU, or (B, 2) ``(stoi, estoi)`` with ``both``; a row with fewer than 30 frames after the
    silent-frame removal scores 1e-5.  ``return_info``: also int32 (B, 3) ``(frames, kept frames, segments)``."""
    if int(fs) not in (16000, 10000):
        raise L.AvvadError("stoi: fs must be 16000 or 10000, got %r" % (fs,))
    if not isinstance(clean, torch.Tensor) or clean.dim() not in (1, 2) or not isinstance(processed, torch.Tensor) \
            or processed.dim() != clean.dim() or processed.shape != clean.shape:
        raise L.AvvadError("stoi: clean and processed must be GPU tensors of one shape (B, L) or (L,), got %s and %s"
                           % (tuple(getattr(clean, "shape", ())), tuple(getattr(processed, "shape", ()))))
    B, Ls = (1, clean.shape[0]) if clean.dim() == 1 else clean.shape
    x, ld_x = _score_rows(clean, "clean", B, Ls)
    y, ld_y = _score_rows(processed, "processed", B, Ls)
    lens32 = None
    if lengths is not None:
        lens32 = lengths_i32(lengths, x.device)
        if lens32.numel() != B:
            raise L.AvvadError("lengths must hold %d values" % B)
    taps = _stoi_taps_on(x.device) if int(fs) == 16000 else None
    which = 3 if both else 2 if extended else 1
    d = torch.empty((B, 2), dtype=torch.float64, device=x.device)
    info = torch.empty((B, 3), dtype=torch.int32, device=x.device)
    ws = _ws(L.lib().avvad_stoi_workspace(B, Ls, int(fs)), x.device)
    L.check(L.lib().avvad_stoi(L.ptr(x), ld_x, L.ptr(y), ld_y, L.ptr(lens32), L.ptr(taps), B, Ls, int(fs), which, L.ptr(d),
                               L.ptr(info), L.ptr(ws), ws.numel() * 4, _stream()), "avvad_stoi")
    out = d if both else d[:, 1] if extended else d[:, 0]
    return (out, info) if return_info else out


class StoiLossFn(torch.autograd.Function):
    """-sum_b d_b (STOI or ESTOI) and its gradient in the processed signal from the same call (avvad_stoi_loss)."""

    @staticmethod
    def forward(ctx, proc, ld_proc, clean, ld_clean, lens32, fs, which):
        B, Ls = proc.shape
        loss = torch.empty(1, dtype=torch.float32, device=proc.device)
        d = torch.empty(B, dtype=torch.float64, device=proc.device)
        dproc = torch.empty(B, Ls, dtype=torch.float32, device=proc.device)
        taps = _stoi_taps_on(proc.device) if fs == 16000 else None
        ws = _ws(L.lib().avvad_stoi_loss_workspace(B, Ls, fs), proc.device)
        L.check(L.lib().avvad_stoi_loss(L.ptr(clean), ld_clean, L.ptr(proc.detach()), ld_proc, L.ptr(lens32), L.ptr(taps), B, Ls, fs,
                                        which, L.ptr(loss), L.ptr(d), None, L.ptr(dproc), Ls, L.ptr(ws), ws.numel() * 4, _stream()),
                "avvad_stoi_loss")
        ctx.save_for_backward(dproc)
        ctx.mark_non_differentiable(d)
        return loss.view(()), d

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dloss, _dd):
        (dproc,) = ctx.saved_tensors
        g = dproc.clone()
        L.check(L.lib().avvad_scale_by_device_scalar(L.ptr(g), L.ptr(_dev(dloss, "dloss").view(1)), g.numel(), _stream()),
                "avvad_scale_by_device_scalar")
        return g, None, None, None, None, None, None


def stoi_loss(processed, clean, lengths=None, fs=16000, extended=False, return_scores=False):
    """``-sum_b STOI_b`` (``extended``: ESTOI) of a ragged batch as a float32 scalar, differentiable in ``processed`` only:
    processed, clean (B, L) (or (L,)) float32 on the GPU, read through their row pitches, cropped to ``lengths``.  The scores
    are ``ops.stoi``'s bit for bit; the keep decision is made from the clean signal and is a constant of the backward, a
    row without a segment scores 1e-5 and has a zero gradient, and the gradient is zero at and behind a row's length.  A
    ``clean`` that requires grad is refused; there is no double backward.  Bit-identical run to run.  ``return_scores``: also
    the (B,) float64 scores."""
    if int(fs) not in (16000, 10000):
        raise L.AvvadError("stoi_loss: fs must be 16000 or 10000, got %r" % (fs,))
    if not isinstance(clean, torch.Tensor) or clean.dim() not in (1, 2) or not isinstance(processed, torch.Tensor) \
            or processed.shape != clean.shape:
        raise L.AvvadError("stoi_loss: processed and clean must be GPU tensors of one shape (B, L) or (L,), got %s and %s"
                           % (tuple(getattr(processed, "shape", ())), tuple(getattr(clean, "shape", ()))))
    if clean.requires_grad:
        raise L.AvvadError("stoi_loss: the clean signal gets no gradient (the keep decision is made from it); detach it")
    if not processed.is_cuda or processed.dtype != torch.float32:
        raise L.AvvadError("processed must be a float32 GPU tensor: the AV-VAD hot path has no CPU fallback")
    y = processed.view(1, -1) if processed.dim() == 1 else processed
    B, Ls = y.shape
    if y.stride(1) != 1 or (B > 1 and y.stride(0) < Ls):
        y = y.contiguous()
    x, ld_x = _score_rows(clean, "clean", B, Ls)
    lens32 = None
    if lengths is not None:
        lens32 = lengths_i32(lengths, y.device)
        if lens32.numel() != B:
            raise L.AvvadError("lengths must hold %d values" % B)
    loss, d = StoiLossFn.apply(y, y.stride(0) if B > 1 else Ls, x, ld_x, lens32, int(fs), 2 if extended else 1)
    return (loss, d) if return_scores else loss


# --------------------------------------------------------------------------- SI-SDR loss (csrc/scores.hip)
class SiSdrLossFn(torch.autograd.Function):
    """-sum_b SI-SDR_b over each row's window, and its gradient in the estimate from the same call (avvad_si_sdr_loss)."""

    @staticmethod
    def forward(ctx, est, ld_est, ref, ld_ref, lens32, head, Lw):
        B, Ls = est.shape
        e, r = est.detach()[:, head:head + Lw], ref[:, head:head + Lw]
        loss = torch.empty(1, dtype=torch.float32, device=est.device)
        ratios = torch.empty(B, dtype=torch.float64, device=est.device)
        dest = torch.empty(B, Ls, dtype=torch.float32, device=est.device)
        ws = _ws(L.lib().avvad_si_sdr_loss_workspace(B, Lw), est.device)
        L.check(L.lib().avvad_si_sdr_loss(L.ptr(e), ld_est, L.ptr(r), ld_ref, L.ptr(lens32), L.ptr(loss), L.ptr(ratios),
                                          L.ptr(dest[:, head:]), Ls, B, Lw, L.ptr(ws), ws.numel() * 4, _stream()), "avvad_si_sdr_loss")
        if head:
            dest[:, :head].zero_()                      # (the call wrote columns head .. L - 1)
        ctx.save_for_backward(dest)
        ctx.mark_non_differentiable(ratios)
        return loss.view(()), ratios

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dloss, _dratios):
        (dest,) = ctx.saved_tensors
        g = dest.clone()
        L.check(L.lib().avvad_scale_by_device_scalar(L.ptr(g), L.ptr(_dev(dloss, "dloss").view(1)), g.numel(), _stream()),
                "avvad_scale_by_device_scalar")
        return g, None, None, None, None, None, None


def si_sdr_loss(est, ref, lengths=None, skip_head=0, skip_tail=0, return_ratios=False):
    """``-sum_b SI-SDR_b`` of a ragged batch as a float32 scalar, differentiable in ``est``: est, ref (B, L) (or (L,)),
    ref rows may be longer.  Row b's window is samples ``[skip_head, lengths[b] - skip_tail)`` (``lengths`` default L);
    the gradient is zero outside it and a row whose window is empty adds nothing.  The trainers skip ``n_fft - hop``
    samples at either end, where ``center=False`` resynthesis divides by a window sum that falls to 1e-10.  The sums are
    those of ``energy_ratios`` (double, fixed order): bit-identical run to run.  ``return_ratios``: also the (B,) float64
    SI-SDR per row in dB (NaN for an empty window)."""
    if not isinstance(est, torch.Tensor) or not est.is_cuda or est.dim() not in (1, 2):
        raise L.AvvadError("est must be a (B, L) or (L,) GPU tensor: the AV-VAD hot path has no CPU fallback")
    e = est.view(1, -1) if est.dim() == 1 else est
    if e.dtype != torch.float32:
        raise L.AvvadError("est must be float32, got %s" % e.dtype)
    if e.stride(1) != 1 or (e.shape[0] > 1 and e.stride(0) < e.shape[1]):
        e = e.contiguous()
    B, Ls = e.shape
    r, ld_r = _score_rows(ref.detach() if isinstance(ref, torch.Tensor) else ref, "ref", B, Ls)
    head, tail = int(skip_head), int(skip_tail)
    if head < 0 or tail < 0:
        raise L.AvvadError("skip_head / skip_tail must not be negative, got %d / %d" % (head, tail))
    lens = [Ls] * B if lengths is None else _ints(lengths, B, Ls, "lengths must hold %d values within 0..%d" % (B, Ls))
    win = [max(0, n - tail - head) for n in lens]
    head = min(head, Ls - 1)
    Lw = Ls - head
    lens32 = torch.tensor(win, dtype=torch.int32).to(e.device)
    loss, ratios = SiSdrLossFn.apply(e, e.stride(0) if B > 1 else Ls, r, ld_r, lens32, head, Lw)
    return (loss, ratios) if return_ratios else loss


def confusion_counts(pred, target, lengths=None, logits=False, counts=None):
    """(B, 4) int64 ``tp, tn, fp, fn`` per row of pred / target (B, T, Y) (or (B, T)), the four sums of ``f1_loss``
    (avvad_confusion_accumulate).  ``pred`` holds 0 / 1, or with ``logits`` the logits (prediction: ``logit > 0``, the
    evaluator's ``sigmoid > 0.5``); frames t >= lengths[b] are not read.  ``counts`` (from an earlier call) is added to."""
    p, y = _dev(pred, "pred"), _dev(target, "target")
    if p.shape != y.shape or p.dim() not in (2, 3):
        raise L.AvvadError("pred and target must both be (B, T, Y) or (B, T), got %s and %s" % (tuple(p.shape), tuple(y.shape)))
    B, T = p.shape[:2]
    Y = p.shape[2] if p.dim() == 3 else 1
    if counts is None:
        counts = torch.zeros(B, 4, dtype=torch.int64, device=p.device)
    elif not isinstance(counts, torch.Tensor) or not counts.is_cuda or counts.dtype != torch.int64 \
            or tuple(counts.shape) != (B, 4) or not counts.is_contiguous():
        raise L.AvvadError("counts must be a contiguous int64 GPU tensor (%d, 4)" % B)
    lens32 = None
    if lengths is not None:
        lens32 = lengths_i32(lengths, p.device)
        if lens32.numel() != B:
            raise L.AvvadError("lengths must hold %d values" % B)
    L.check(L.lib().avvad_confusion_accumulate(L.ptr(p), 1 if logits else 0, L.ptr(y), L.ptr(lens32), L.ptr(counts), B, T, Y,
                                               _stream()), "avvad_confusion_accumulate")
    return counts


def f1_from_counts(counts, eps=1e-8):
    """(B, 4) float32 ``accuracy, precision, recall, f1`` from (B, 4) ``tp, tn, fp, fn``: ``f1_loss``'s own float32
    expressions (packages/models/utils.py:191-200) on the counts, row by row the values ``f1_loss`` returns."""
    tp, tn, fp, fn = (counts[..., k].to(torch.float32) for k in range(4))
    accuracy = (tp + tn) / (tp + tn + fp + fn + eps)
    precision = tp / (tp + fp + eps)
    recall = tp / (tp + fn + eps)
    f1 = 2 * (precision * recall) / (precision + recall + eps)
    return torch.stack([accuracy, precision, recall, f1], dim=-1)


# --------------------------------------------------------------------------- mixing at a target SNR (csrc/mix.hip, no gradient)
MIX_CHUNK = L.MIX_CHUNK          # samples of one energy partial of the mix (include/avvad.h AVVAD_MIX_CHUNK)


class NoiseBank:
    """Noise clips as ``avvad_mix`` reads them: ``data`` one flat float32 tensor on ``device`` that holds the clips back to
    back, ``clip_off`` (int64) / ``clip_len`` (int32) device arrays, and the same numbers on the host -- ``offsets`` /
    ``lengths``, Python lists -- for validation and for drawing starts.  ``clips``: a list of 1-D float tensors or arrays,
    each of at least one sample."""

    def __init__(self, clips, device):
        clips = [torch.as_tensor(c).detach().to("cpu", torch.float32) for c in clips]
        if not clips or any(c.dim() != 1 or c.numel() < 1 for c in clips):
            raise L.AvvadError("a noise bank holds at least one clip, each a 1-D signal of at least one sample")
        self.lengths = [int(c.numel()) for c in clips]
        if max(self.lengths) >= 2 ** 31:
            raise L.AvvadError("a noise clip holds fewer than 2^31 samples")
        self.offsets = [0]
        for n in self.lengths[:-1]:
            self.offsets.append(self.offsets[-1] + n)
        self.K = len(clips)
        self.device = torch.device(device)
        self.data = torch.cat(clips).to(self.device)
        self.clip_off = torch.tensor(self.offsets, dtype=torch.int64).to(self.device)
        self.clip_len = torch.tensor(self.lengths, dtype=torch.int32).to(self.device)

    def __len__(self):
        return self.K


def mix_ratio(snr_db):
    """The linear power ratio ``10 ** (snr_db / 10)`` ``avvad_mix`` takes, as a float64 computed on the host."""
    import numpy as np
    with np.errstate(over="ignore"):         # (an SNR beyond a double's range gives inf, which ``mix`` refuses)
        return np_power10(float(snr_db) / 10.0)


def mix(clean, lengths, bank, clip, start, snr_db, return_noise=False, return_info=False, out=None, noise_out=None):
    """Clean speech and noise mixed at a target SNR on the GPU (avvad_mix): ``clean`` (B, L) (or (L,)) float32 rows with
    ``lengths`` real samples each (None: L), ``bank`` a ``NoiseBank``; row b takes clip ``clip[b]`` read circularly from
    ``start[b]`` and is scaled by ``g_b`` so that ``sum clean^2 / sum (g_b noise)^2 = 10 ** (snr_db[b] / 10)`` over the
    row's samples.  ``clip``, ``start``, ``snr_db``: host lists or tensors of B entries (``snr_db`` may be one number),
    validated here: ``0 <= clip < len(bank)``, ``0 <= start < `` the clip's length, a finite ``snr_db``.  Returns
    ``noisy`` (B, L) -- ``clean + g noise``, exact zeros behind each length -- then ``noise`` (B, L), the scaled noise
    ``g_b n``, with ``return_noise``, then ``{"gain" (B,) float32, "energies" (B, 2) float64 (speech, unscaled noise),
    "peak" (B,) float32 = ops.peak(noisy)}`` with ``return_info``.  A row whose speech or noise segment is silent, or whose
    length is 0, has gain 0 and ``noisy == clean``.  Nothing is peak-normalised here.  ``clean`` is read through its
    strides; ``out`` / ``noise_out``: float32 GPU tensors of B rows of at least L unit-stride samples to write into
    (columns from L on are left alone), e.g. column slices of wider tensors."""
    if not isinstance(clean, torch.Tensor) or clean.dim() not in (1, 2):
        raise L.AvvadError("clean must be a (B, L) or (L,) GPU tensor: the AV-VAD hot path has no CPU fallback")
    if not isinstance(bank, NoiseBank):
        raise L.AvvadError("bank must be an ops.NoiseBank")
    B, Ls = (1, clean.shape[0]) if clean.dim() == 1 else clean.shape
    s, ld_s = _score_rows(clean, "clean", B, Ls)
    if bank.data.device != s.device:
        raise L.AvvadError("the noise bank must live on the GPU of the clean batch (%s), it is on %s" % (s.device, bank.data.device))
    lens = [Ls] * B if lengths is None else _ints(lengths, B, Ls, "lengths must hold %d values within 0..%d" % (B, Ls))
    clips = _ints(clip, B, bank.K - 1, "clip must hold %d clip indices within 0..%d" % (B, bank.K - 1))
    starts = _ints(start, B, None, "start must hold %d values that are not negative" % B)
    for b, (k, st) in enumerate(zip(clips, starts)):
        if st >= bank.lengths[k]:
            raise L.AvvadError("start[%d] = %d lies outside clip %d of %d samples" % (b, st, k, bank.lengths[k]))
    snr = snr_db.tolist() if isinstance(snr_db, torch.Tensor) else snr_db
    snr = [float(snr)] * B if isinstance(snr, (int, float)) else [float(v) for v in snr]
    if len(snr) != B or not all(math.isfinite(v) for v in snr):
        raise L.AvvadError("snr_db must hold %d finite values" % B)
    ratio = [mix_ratio(v) for v in snr]
    if not all(math.isfinite(r) and r > 0.0 for r in ratio):
        raise L.AvvadError("snr_db must stay within what a float64 power ratio can hold")

    def dest(t, name, want):
        if t is None:
            return (torch.empty(B, Ls, dtype=torch.float32, device=s.device), Ls) if want else (None, 0)
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.device != s.device:
            raise L.AvvadError("%s must be a float32 GPU tensor on the clean batch's device" % name)
        t2 = t.view(1, -1) if t.dim() == 1 else t
        if t2.dim() != 2 or t2.shape[0] != B or t2.shape[1] < Ls or t2.stride(1) != 1 or (B > 1 and t2.stride(0) < Ls):
            raise L.AvvadError("%s must hold %d rows of at least %d unit-stride samples" % (name, B, Ls))
        return t2[:, :Ls], (t2.stride(0) if B > 1 else Ls)
    noisy, ld_y = dest(out, "out", True)
    noise, ld_z = dest(noise_out, "noise_out", return_noise)
    gain = peak_ = energies = None
    if return_info:
        gain = torch.empty(B, dtype=torch.float32, device=s.device)
        peak_ = torch.empty(B, dtype=torch.float32, device=s.device)
        energies = torch.empty(B, 2, dtype=torch.float64, device=s.device)
    # the per-row arguments in ONE host-to-device copy: B doubles (8-byte aligned at the block's base), then 3 x B int32
    import numpy as np
    host = np.empty(20 * B, dtype=np.uint8)
    host[:8 * B].view(np.float64)[:] = ratio
    host[8 * B:].view(np.int32)[:] = lens + clips + starts
    args = torch.from_numpy(host).to(s.device)
    rat, idx = args[:8 * B].view(torch.float64), args[8 * B:].view(torch.int32).view(3, B)
    ws = _ws(L.lib().avvad_mix_workspace(B, Ls), s.device)
    L.check(L.lib().avvad_mix(L.ptr(s), ld_s, L.ptr(idx[0]), L.ptr(bank.data), bank.data.numel(), L.ptr(bank.clip_off),
                              L.ptr(bank.clip_len), bank.K, L.ptr(idx[1]), L.ptr(idx[2]), L.ptr(rat), L.ptr(noisy), ld_y,
                              L.ptr(noise), ld_z, L.ptr(gain), L.ptr(energies), L.ptr(peak_), B, Ls, L.ptr(ws), ws.numel() * 4,
                              _stream()), "avvad_mix")
    if clean.dim() == 1 and out is None:
        noisy = noisy.view(-1)
    if clean.dim() == 1 and noise is not None and noise_out is None:
        noise = noise.view(-1)
    res = (noisy,)
    if noise is not None:
        res += (noise,)
    if return_info:
        res += ({"gain": gain, "energies": energies, "peak": peak_},)
    return res[0] if len(res) == 1 else res


# --------------------------------------------------------------------------- training labels from clean speech (no gradient)
_CENTER ={"reflect": 1, "constant": 2}


def target_frames(L, fs=16e3, wlen_sec=64e-3, hop_percent=0.25, center=False, pad_at_end=True):
    """(samples after the end pad, frame count) of ``clean_speech_VAD`` (packages/processing/target.py:28-46): one hop of
    zeros when ``ceil(L/fs/wlen_sec/hop_percent) != int(...)``, evaluated exactly as the reference writes it, then
    ``n_fft//2`` per side when ``center``, then ``librosa.util.frame``'s ``1 + (len - n_fft)//hop`` frames."""
    nfft = int(wlen_sec * fs)
    hop = int(hop_percent * nfft)
    n = int(L)
    if pad_at_end and _end_pad(n, fs, wlen_sec, hop_percent):
        n += hop
    total = n + (2 * (nfft // 2) if center else 0)
    if total < nfft:
        raise AvvadError("utterance of %d samples is shorter than one %d-sample frame" % (int(L), nfft))
    return n, 1 + (total - nfft) // hop


def _target_call(wave, sample_lengths, fs, wlen_sec, hop_percent, center, pad_mode, pad_at_end, vad_threshold, eps, ibm_threshold):
    w, w2 = _wave2d(wave)
    B, Lp = w2.shape
    lens = _ints(sample_lengths, B, Lp, "sample_lengths must hold %d lengths within 0..%d" % (B, Lp))
    if center and pad_mode not in _CENTER:
        raise L.AvvadError("pad_mode %r: the GPU labels implement 'reflect' and 'constant'" % (pad_mode,))
    if wlen_sec * fs != int(wlen_sec * fs):
        raise ValueError("wlen_sample of STFT is not an integer.")
    nfft = int(wlen_sec * fs)
    hop = int(hop_percent * nfft)
    pads, frames = zip(*[target_frames(n, fs, wlen_sec, hop_percent, center, pad_at_end) for n in lens])
    if center and pad_mode == "reflect" and min(pads) <= nfft // 2:
        raise L.AvvadError("reflect padding of %d samples needs utterances longer than that" % (nfft // 2))
    T = max(frames)
    d = L.TargetDesc(B, Lp, nfft, hop, T, _CENTER[pad_mode] if center else 0, float(eps), float(np_power10(vad_threshold)),
                     float(np_power10(-ibm_threshold / 20.0)))
    ws = _ws(L.lib().avvad_target_workspace(C.byref(d)), w.device)
    dev_counts = torch.tensor([list(pads), list(frames)], dtype=torch.int32).to(w.device)
    return w2, d, ws, dev_counts, torch.LongTensor(frames)


def np_power10(x):
    """``np.power(10, x)`` of the reference as a float64 (a Python float: the same IEEE double)."""
    import numpy as np
    return float(np.power(10, np.float64(x)))


def speech_targets(clean, sample_lengths, labels="vad_labels", robust=False, fs=16e3, wlen_sec=64e-3, hop_percent=0.25,
                   center=False, pad_mode="reflect", pad_at_end=True, vad_threshold=1.70, eps=1e-8, ibm_threshold=50):
    """Training labels of a ragged batch of clean utterances, computed on the GPU (packages/processing/target.py):
    clean (B, L) zero-padded rows (or (L,)), ``sample_lengths`` the B real lengths.  ``labels='vad_labels'``: the
    framed-energy VAD, target (B, T, 1); ``'ibm_labels'``: the ideal binary mask, target (B, T, n_fft/2+1) (``center``
    False only), times the VAD when ``robust``.  Defaults are the training pipeline's (create_audio_train_files.py:44-60).
    Returns (frame_lengths LongTensor (B,) on the host, target on the GPU); frames t >= T_b are zero -- the layout of
    the collates, ready for ``forward_batch``.  The waveform is taken as given (callers peak-normalise, as the reference
    does before calling target.py)."""
    if labels not in ("vad_labels", "ibm_labels"):
        raise L.AvvadError("labels must be 'vad_labels' or 'ibm_labels', got %r" % (labels,))
    w2, d, ws, cnt, frames = _target_call(clean, sample_lengths, fs, wlen_sec, hop_percent, center, pad_mode, pad_at_end,
                                          vad_threshold, eps, ibm_threshold)
    if labels == "vad_labels":
        out = torch.empty(d.B, d.T, 1, dtype=torch.float32, device=w2.device)
        L.check(L.lib().avvad_target_vad(L.ptr(w2), L.ptr(cnt[0]), L.ptr(cnt[1]), L.ptr(out), C.byref(d), L.ptr(ws), ws.numel() * 4,
                                         _stream()), "avvad_target_vad")
        return frames, out
    if center or d.n_fft % 32:
        raise L.AvvadError("IBM labels from a waveform need center=False and an FFT length that is a multiple of 32")
    out = torch.empty(d.B, d.T, d.n_fft // 2 + 1, dtype=torch.float32, device=w2.device)
    L.check(L.lib().avvad_target_ibm(L.ptr(w2), L.ptr(cnt[0]), L.ptr(cnt[1]), int(bool(robust)), L.ptr(out), C.byref(d), L.ptr(ws),
                                     ws.numel() * 4, _stream()), "avvad_target_ibm")
    return frames, out


def ibm_from_spectrum(spec, eps=1e-8, ibm_threshold=50, vad=None):
    """``clean_speech_IBM`` of one given spectrum on the GPU: ``spec`` a complex (F, T) tensor or its real (F, T, 2) view
    (the legacy layout ``stft_pytorch`` returns), read in place through its strides.  ``vad`` (T,) multiplies each frame
    (``noise_robust_clean_speech_IBM``).  Returns the (F, T) mask."""
    if isinstance(spec, torch.Tensor) and spec.is_complex():
        if spec.dtype != torch.complex64:
            raise L.AvvadError("spectrum must be complex64, got %s" % spec.dtype)
        spec = torch.view_as_real(spec)
    if not isinstance(spec, torch.Tensor) or not spec.is_cuda or spec.dtype != torch.float32:
        raise L.AvvadError("spectrum must be a complex64 or float32 (F, T, 2) GPU tensor")
    if spec.dim() != 3 or spec.shape[2] != 2 or spec.stride(2) != 1 or spec.shape[0] < 2 or spec.shape[1] < 1:
        raise L.AvvadError("spectrum must be (F >= 2, T, 2) with (re, im) adjacent, got shape %s strides %s"
                           % (tuple(spec.shape), spec.stride()))
    if spec.stride(0) % 2 or spec.stride(1) % 2 or spec.stride(0) <= 0 or spec.stride(1) <= 0:
        spec = spec.contiguous()
    F, T = spec.shape[0], spec.shape[1]
    d = L.TargetDesc(1, T, 2 * (F - 1), 1, T, 0, float(eps), 1.0, float(np_power10(-ibm_threshold / 20.0)))
    ws = _ws(8, spec.device)
    if vad is not None:
        vad = _dev(vad, "vad").reshape(-1)
        if vad.numel() != T:
            raise L.AvvadError("vad holds %d frames, the spectrum %d" % (vad.numel(), T))
    out = torch.empty(F, T, dtype=torch.float32, device=spec.device)
    L.check(L.lib().avvad_target_ibm_from_spectrum(L.ptr(spec), spec.stride(1), spec.stride(0), L.ptr(vad), L.ptr(out), C.byref(d),
                                                   L.ptr(ws), ws.numel() * 4, _stream()), "avvad_target_ibm_from_spectrum")
    return out


# --------------------------------------------------------------------------- noise-aware masks from speech and noise (no gradient)
NOISE_AWARE_OUTPUTS = ("speech", "noise", "irm")


def voiced_unvoiced_characteristic(F):
    """``_voiced_unvoiced_split_characteristic`` of the reference (packages/processing/target.py:110-149) -> (voiced,
    unvoiced), float64 (F,): two weights per bin that cross over around bin 200 on a 99-bin raised cosine (bins 149 ..
    247), voiced rising from 0 over bins 3 .. 7, unvoiced falling to 0 over bins 499 .. 503.  Every value is formed by the
    reference's operations in its order, so the tables equal its bits.  The fixed bins need F >= 505."""
    import numpy as np
    if F < 505:
        raise ValueError("the voiced / unvoiced characteristic has fixed bins up to 503 and needs F >= 505, got %d" % F)
    split, width, fast_width, low, high = 200, 99, 5, 4, 500
    slow = 0.5 * (1 + np.cos(np.pi / (width - 1) * np.arange(0, width)))
    fast = (np.cos(np.pi / (fast_width - 1) * np.arange(0, fast_width)) + 1) / 2
    first = int(split - width / 2) - 1                  # 149: where the cross-over starts
    voiced, unvoiced = np.ones(F), np.ones(F)
    voiced[first:first + width] = slow
    voiced[first + width:] = 0
    voiced[:low] = 0
    voiced[low - 1:low - 1 + fast_width] = 1 - fast
    unvoiced[first:first + width] = 1 - slow
    unvoiced[:first + 1] = 0
    unvoiced[high - 1:] = 0
    unvoiced[high - 1:high - 1 + fast_width] = fast
    return voiced, unvoiced


def noise_aware_tables(F, threshold_unvoiced_speech=5, threshold_voiced_speech=0, threshold_unvoiced_noise=-10,
                       threshold_voiced_noise=-10):
    """(c_speech, c_noise), float64 (F,): the per-bin power ratios ``10 ** (threshold_f / 10)`` that ``noise_aware_IBM``
    divides the speech power by (target.py:175-186), on the host.  As there, the noise row weights ``voiced`` with
    ``threshold_unvoiced_noise`` and ``unvoiced`` with ``threshold_voiced_noise``."""
    import numpy as np
    voiced, unvoiced = voiced_unvoiced_characteristic(F)
    thr_speech = threshold_voiced_speech * voiced + threshold_unvoiced_speech * unvoiced
    thr_noise = threshold_unvoiced_noise * voiced + threshold_voiced_noise * unvoiced
    return np.power(10, (thr_speech / 10)), np.power(10, (thr_noise / 10))


def _na_args(F, B, device, outputs, peak, thresholds, low_cut, high_cut):
    """What the two noise-aware calls share: the tables on the device (one copy), the checked cuts, peak and outputs."""
    import numpy as np
    outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    if not outputs or any(o not in NOISE_AWARE_OUTPUTS for o in outputs) or len(set(outputs)) != len(outputs):
        raise L.AvvadError("outputs: one or more of %s, got %r" % (", ".join(NOISE_AWARE_OUTPUTS), outputs))
    low_cut, high_cut = int(low_cut), int(high_cut)
    if low_cut < 1 or high_cut > F:
        raise L.AvvadError("low_cut %d / high_cut %d: 1 <= low_cut and high_cut <= %d bins" % (low_cut, high_cut, F))
    tables = torch.from_numpy(np.stack(noise_aware_tables(F, *thresholds))).to(device)
    if peak is not None:
        peak = _dev(peak, "peak").reshape(-1)
        if peak.numel() != B:
            raise L.AvvadError("peak holds %d values, the batch %d rows" % (peak.numel(), B))
    return outputs, tables, peak, low_cut, high_cut


def noise_aware_targets(speech, noise, sample_lengths, peak=None, outputs=("speech",), threshold_unvoiced_speech=5,
                        threshold_voiced_speech=0, threshold_unvoiced_noise=-10, threshold_voiced_noise=-10, low_cut=5,
                        high_cut=500, floor=0.005, fs=16e3, wlen_sec=64e-3, hop_percent=0.25, pad_at_end=True):
    """Noise-aware labels of a ragged batch of mixtures from their two components (avvad_target_noise_aware): ``speech``
    and ``noise`` (B, L) zero-padded rows (or (L,)) -- for ``ops.mix``, the clean wave and the scaled noise ``g n`` --
    ``sample_lengths`` the B real lengths, ``peak`` (B,) what both are divided by (the mixture's peak puts them on the
    scale of the normalised mixture; it matters for the ``floor`` only) or None.  ``outputs``: any of "speech" (the
    speech mask of ``noise_aware_IBM``, target.py:151-202), "noise" (its noise mask) and "irm" (the ideal ratio mask
    ``|S|^2 / (|S|^2 + |N|^2)``); the six thresholds and cuts default as in the reference.  Framing as ``speech_targets``
    with ``center=False``.  Returns (frame_lengths LongTensor (B,) on the host, {name: (B, T, n_fft/2+1) float32}); frames
    t >= T_b are zero."""
    w, w2 = _wave2d(speech)
    _, n2 = _wave2d(noise)
    if n2.shape != w2.shape or n2.device != w2.device:
        raise L.AvvadError("speech %s and noise %s must have one shape and one device" % (tuple(w2.shape), tuple(n2.shape)))
    B, Lp = w2.shape
    lens = _ints(sample_lengths, B, Lp, "sample_lengths must hold %d lengths within 0..%d" % (B, Lp))
    if wlen_sec * fs != int(wlen_sec * fs):
        raise ValueError("wlen_sample of STFT is not an integer.")
    nfft = int(wlen_sec * fs)
    hop = int(hop_percent * nfft)
    if nfft % 32:
        raise L.AvvadError("noise-aware labels need an FFT length that is a multiple of 32")
    F = nfft // 2 + 1
    thresholds = (threshold_unvoiced_speech, threshold_voiced_speech, threshold_unvoiced_noise, threshold_voiced_noise)
    outputs, tables, peak, low_cut, high_cut = _na_args(F, B, w2.device, outputs, peak, thresholds, low_cut, high_cut)
    pads, frames = zip(*[target_frames(n, fs, wlen_sec, hop_percent, False, pad_at_end) for n in lens])
    T = max(frames)
    d = L.TargetDesc(B, Lp, nfft, hop, T, 0, 0.0, 1.0, 1.0)
    ws = _ws(L.lib().avvad_target_noise_aware_workspace(C.byref(d)), w2.device)
    cnt = torch.tensor([list(pads), list(frames)], dtype=torch.int32).to(w2.device)
    res = {o: torch.empty(B, T, F, dtype=torch.float32, device=w2.device) for o in outputs}
    L.check(L.lib().avvad_target_noise_aware(L.ptr(w2), L.ptr(n2), L.ptr(cnt[0]), L.ptr(cnt[1]), L.ptr(peak), L.ptr(tables[0]),
                                             L.ptr(tables[1]), low_cut, high_cut, float(floor), L.ptr(res.get("speech")),
                                             L.ptr(res.get("noise")), L.ptr(res.get("irm")), C.byref(d), L.ptr(ws), ws.numel() * 4,
                                             _stream()), "avvad_target_noise_aware")
    return torch.LongTensor(frames), res


def _spectrum_view(spec, name):
    """A complex64 (T, F) / (B, T, F) GPU tensor or its float32 (..., 2) view -> (the (B, T, F, 2) view read through its
    strides, batched?)"""
    if isinstance(spec, torch.Tensor) and spec.is_complex():
        if spec.dtype != torch.complex64:
            raise L.AvvadError("%s must be complex64, got %s" % (name, spec.dtype))
        spec = torch.view_as_real(spec)
    if not isinstance(spec, torch.Tensor) or not spec.is_cuda or spec.dtype != torch.float32:
        raise L.AvvadError("%s must be a complex64 or float32 (..., 2) GPU tensor" % name)
    if spec.dim() not in (3, 4) or spec.shape[-1] != 2 or 0 in spec.shape:
        raise L.AvvadError("%s must be (T, F) or (B, T, F) complex, or the (..., 2) real view, got shape %s" % (name, tuple(spec.shape)))
    batched = spec.dim() == 4
    s4 = spec if batched else spec.unsqueeze(0)
    st = s4.stride()
    if st[3] != 1 or any(v % 2 or v <= 0 for v in st[1:3]) or (s4.shape[0] > 1 and (st[0] % 2 or st[0] <= 0)) or s4.data_ptr() % 8:
        s4 = s4.contiguous()
    return s4, batched


def noise_aware_from_spectrum(X, N=None, n_frames=None, peak=None, outputs=("speech", "noise"), threshold_unvoiced_speech=5,
                              threshold_voiced_speech=0, threshold_unvoiced_noise=-10, threshold_voiced_noise=-10, low_cut=5,
                              high_cut=500, floor=0.005, noise_psd=10.0):
    """The masks of ``noise_aware_targets`` from given spectra (avvad_target_noise_aware_from_spectrum): ``X`` (speech)
    and ``N`` (noise) complex64 (T, F) or (B, T, F) GPU tensors, or their float32 (..., 2) views, each read in place
    through its strides -- a transposed legacy (F, T, 2) view or a column slice of a wider tensor is not copied.
    ``N`` None: the noise power is the constant ``noise_psd`` in every cell (``threshold_IBM``, target.py:205-251).
    ``n_frames``: B frame counts (frames behind them are zero) or None; ``peak`` as in ``noise_aware_targets``.
    Returns {name: (T, F) or (B, T, F) float32}."""
    x4, batched = _spectrum_view(X, "X")
    B, T, F = x4.shape[:3]
    n4 = None
    if N is not None:
        n4, _ = _spectrum_view(N, "N")
        if n4.shape != x4.shape or n4.device != x4.device:
            raise L.AvvadError("X %s and N %s must have one shape and one device" % (tuple(x4.shape), tuple(n4.shape)))
    thresholds = (threshold_unvoiced_speech, threshold_voiced_speech, threshold_unvoiced_noise, threshold_voiced_noise)
    outputs, tables, peak, low_cut, high_cut = _na_args(F, B, x4.device, outputs, peak, thresholds, low_cut, high_cut)
    cnt = None
    if n_frames is not None:
        cnt = torch.tensor(_ints(n_frames, B, T, "n_frames must hold %d counts within 0..%d" % (B, T)), dtype=torch.int32).to(x4.device)
    res = {o: torch.empty(B, T, F, dtype=torch.float32, device=x4.device) for o in outputs}
    sx = (x4.stride(0) if B > 1 else 0,) + tuple(x4.stride()[1:3])          # (one row: its batch stride is not read)
    sn = ((n4.stride(0) if B > 1 else 0,) + tuple(n4.stride()[1:3])) if n4 is not None else (0, 0, 0)
    L.check(L.lib().avvad_target_noise_aware_from_spectrum(
        L.ptr(x4), sx[0], sx[1], sx[2], L.ptr(n4), sn[0], sn[1], sn[2], L.ptr(cnt), L.ptr(peak), L.ptr(tables[0]), L.ptr(tables[1]),
        low_cut, high_cut, float(floor), float(noise_psd), L.ptr(res.get("speech")), L.ptr(res.get("noise")), L.ptr(res.get("irm")),
        B, T, F, _stream()), "avvad_target_noise_aware_from_spectrum")
    return res if batched else {o: v[0] for o, v in res.items()}


# --------------------------------------------------------------------------- mask-regression losses (csrc/spectral_loss.hip)
SPECTRAL_CHUNK = L.SPECTRAL_CHUNK    # cells of one partial of the loss pass (include/avvad.h AVVAD_SPECTRAL_CHUNK)
SPECTRAL_KINDS = {"mask": 0, "signal": 1, "spectrum": 2}


class SpectralLossFn(torch.autograd.Function):
    """The summed mask-regression loss of a ragged batch and its gradient in ``pred`` from the same call
    (avvad_spectral_loss); without a gradient to compute (``pred`` needs none) the kernel writes none."""

    @staticmethod
    def forward(ctx, pred, kind, pred_mode, target, mix4, speech4, lens32):
        B, T, F = pred.shape
        p = pred.detach()
        loss = torch.empty(1, dtype=torch.float32, device=p.device)
        rows = torch.empty(B, dtype=torch.float64, device=p.device)
        dpred = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        ws = _ws(L.lib().avvad_spectral_loss_workspace(B, T, F), p.device)

        def strides(s4):                    # (one row: its batch stride is not read)
            return (0, 0, 0) if s4 is None else ((s4.stride(0) if B > 1 else 0,) + tuple(s4.stride()[1:3]))
        L.check(L.lib().avvad_spectral_loss(L.ptr(p), pred_mode, kind, L.ptr(target), L.ptr(mix4), *strides(mix4), L.ptr(speech4),
                                            *strides(speech4), L.ptr(lens32), L.ptr(loss), L.ptr(rows), L.ptr(dpred), B, T, F,
                                            L.ptr(ws), ws.numel() * 4, _stream()), "avvad_spectral_loss")
        if dpred is not None:
            ctx.save_for_backward(dpred)
        ctx.mark_non_differentiable(rows)
        return loss.view(()), rows

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dloss, _drows):
        (dpred,) = ctx.saved_tensors
        g = dpred.clone()
        L.check(L.lib().avvad_scale_by_device_scalar(L.ptr(g), L.ptr(_dev(dloss, "dloss").view(1)), g.numel(), _stream()),
                "avvad_scale_by_device_scalar")
        return g, None, None, None, None, None, None


def spectral_loss(pred, kind, target=None, mix=None, speech=None, lengths=None, pred_mode=2, return_rows=False):
    """The mask-regression losses of ``packages/models/utils.py:151-162`` for a ragged batch, as a float32 scalar that is
    differentiable in ``pred`` (B, T, F) (or one utterance (T, F)).  ``pred_mode`` 2: ``pred`` holds logits and the mask is
    ``m = sigmoid(pred)``; 1: ``pred`` is the mask itself (``ops.istft``'s numbers).  ``kind``:
      "mask"      ``(y - m)^2``                 ``target`` y, float32, shaped like ``pred``
      "signal"    ``((y - m) |X|)^2``           ``target`` and ``mix`` X
      "spectrum"  ``|S - m X|^2`` (complex)     ``mix`` X and ``speech`` S
    summed over the bins, averaged over each row's first ``lengths[b]`` frames (None: T) and summed over the batch, like
    ``masked_bce`` and ``si_sdr_loss``; a row of length 0 adds nothing.  ``mix`` / ``speech``: complex64 (T, F) or
    (B, T, F) GPU tensors or their float32 (..., 2) views -- ``ops.stft_complex``'s (B, T, F, 2), a transposed legacy
    (F, T, 2) view -- read in place through their strides.  ``target``, ``mix`` and ``speech`` are data: no gradient.
    Double sums in a fixed order: bit-identical run to run, and a row's value and gradient do not depend on its batch.
    ``return_rows``: also the (B,) float64 per-row losses."""
    if kind not in SPECTRAL_KINDS:
        raise L.AvvadError("kind %r: one of %s" % (kind, ", ".join(SPECTRAL_KINDS)))
    if pred_mode not in (1, 2):
        raise L.AvvadError("pred_mode must be 1 (pred is the mask) or 2 (pred holds logits), got %r" % (pred_mode,))
    if not isinstance(pred, torch.Tensor) or not pred.is_cuda or pred.dim() not in (2, 3) or 0 in pred.shape:
        raise L.AvvadError("pred must be a (B, T, F) or (T, F) GPU tensor: the AV-VAD hot path has no CPU fallback")
    if pred.dtype != torch.float32:
        raise L.AvvadError("pred must be float32, got %s" % pred.dtype)
    k = SPECTRAL_KINDS[kind]
    p = (pred.unsqueeze(0) if pred.dim() == 2 else pred).contiguous()
    B, T, F = p.shape
    y = x4 = s4 = None
    if k < 2:
        if target is None:
            raise L.AvvadError("kind %r needs target" % kind)
        y = _dev(target.detach() if isinstance(target, torch.Tensor) else target, "target")
        if y.numel() != p.numel() or tuple(y.shape[-2:]) != (T, F) or y.device != p.device:
            raise L.AvvadError("target %s must have the shape and device of pred %s" % (tuple(y.shape), tuple(pred.shape)))
    for name, spec, need in (("mix", mix, k >= 1), ("speech", speech, k == 2)):
        if not need:
            continue
        if spec is None:
            raise L.AvvadError("kind %r needs %s" % (kind, name))
        v4, _ = _spectrum_view(spec.detach() if isinstance(spec, torch.Tensor) else spec, name)
        if tuple(v4.shape[:3]) != (B, T, F) or v4.device != p.device:
            raise L.AvvadError("%s %s must hold the (B, T, F) = %s complex bins of pred, on its device" % (name, tuple(v4.shape), (B, T, F)))
        if name == "mix":
            x4 = v4
        else:
            s4 = v4
    lens32 = None
    if lengths is not None:
        lens32 = lengths_i32(lengths, p.device)
        if lens32.numel() != B:
            raise L.AvvadError("lengths must hold %d values, got %d" % (B, lens32.numel()))
    loss, rows = SpectralLossFn.apply(p, k, int(pred_mode), y, x4, s4, lens32)
    return (loss, rows) if return_rows else loss


# --------------------------------------------------------------------------- video front-end: lip DCT frames (no gradient)
LIP_W = LIP_H = 67


def lip_rate(fs=16000, hop=256, fps_in=30):
    """(p, q): output frames per input frame ``fs / (hop * fps_in)`` in lowest terms -- 25 / 12 for the defaults."""
    from fractions import Fraction
    r = Fraction(fs).limit_denominator(10 ** 6) / (Fraction(hop).limit_denominator(10 ** 6) * Fraction(fps_in).limit_denominator(10 ** 6))
    if r <= 0:
        raise L.AvvadError("fs, hop and fps_in must be positive")
    return r.numerator, r.denominator


def lip_frame_starts(N, fs=16000, hop=256, fps_in=30):
    """``[s(0), ..., s(N)]``: output frame ``k`` shows input frame ``i`` for ``s(i) <= k < s(i+1)``, with
    ``s(i) = round_half_away(i p / q) = (2 i p + q) // (2 q)`` -- our reading of the nearest-timestamp rule of ffmpeg's
    ``fps`` filter (create_video_train_files_upsampled.py:122).  Integer arithmetic only."""
    p, q = lip_rate(fs, hop, fps_in)
    return [(2 * i * p + q) // (2 * q) for i in range(int(N) + 1)]


def lip_out_frames(N, fs=16000, hop=256, fps_in=30):
    """``T_video = s(N)``: frames of an utterance of ``N`` coefficient frames after the rate conversion."""
    p, q = lip_rate(fs, hop, fps_in)
    return (2 * int(N) * p + q) // (2 * q)


def lip_decode(coef, n_in, n_out=None, quantize=True, acc=None, mean=None, std=None, eps=1e-8, fs=16000, hop=256, fps_in=30):
    """Lip-region DCT coefficients -> video crops at the STFT's frame rate (avvad_lip_decode; what the reference's
    ``process_write_video`` computes offline, create_video_train_files_upsampled.py:105-173): 2-D inverse DCT of every
    frame, ``(A - min over the utterance) / (largest per-frame range) * 255``, ``rot90(., 3)``, clip to [0, 255] and round
    towards zero (``quantize``; the codec round trip of the reference is not modelled), each input frame repeated over the
    output frames ``lip_frame_starts`` assigns to it.

    ``coef``: float32 on the GPU, a padded batch (B, Nmax, 4489) or the utterances' rows packed one after the other
    (sum N_b, 4489); ``n_in`` the B frame counts.  ``n_out`` (optional, B values: the label frame counts) caps the output
    lengths.  ``acc`` (``ops.stats_new(1, device)``) receives the written frames' sum / sum of squares / pixel count --
    what ``accumulate_stats(acc, video.view(B, T, 4489), lengths, nstat=1)`` would add, before any standardisation;
    ``mean`` / ``std`` (one value each) store ``(x - mean) / (std + eps)``, the standardisation of ``Stats.video``.
    An utterance of constant frames (range 0) is written as 0.  Returns (video (B, Tmax, 67, 67) on the GPU with frames
    ``k >= lengths[b]`` zero, lengths LongTensor (B,) on the host)."""
    c = _dev(coef, "coef")
    npix = LIP_W * LIP_H
    if c.dim() not in (2, 3) or c.shape[-1] != npix:
        raise L.AvvadError("coef must be (B, Nmax, %d) or (sum N, %d), got shape %s" % (npix, npix, tuple(c.shape)))
    n_in = _ints(n_in)
    B = len(n_in)
    if B == 0 or min(n_in) < 0:
        raise L.AvvadError("n_in must hold at least one non-negative frame count")
    if c.dim() == 3:
        if c.shape[0] != B or max(n_in) > c.shape[1]:
            raise L.AvvadError("n_in must hold %d counts within 0..%d" % (c.shape[0], c.shape[1]))
        starts = [b * c.shape[1] for b in range(B)]
    else:
        starts = [sum(n_in[:b]) for b in range(B)]
        if sum(n_in) > c.shape[0]:
            raise L.AvvadError("n_in counts %d frames, coef holds %d" % (sum(n_in), c.shape[0]))
    rows = c.numel() // npix
    p, q = lip_rate(fs, hop, fps_in)
    lens = [(2 * n * p + q) // (2 * q) for n in n_in]
    if n_out is not None:
        n_out = _ints(n_out)
        if len(n_out) != B:
            raise L.AvvadError("n_out must hold %d values, got %d" % (B, len(n_out)))
        lens = [min(t, max(m, 0)) for t, m in zip(lens, n_out)]
    if acc is not None and _acc_nstat(acc) != 1:
        raise L.AvvadError("the video statistics are one scalar pair: acc must come from stats_new(1, device)")
    if (mean is None) != (std is None):
        raise L.AvvadError("the fused standardisation needs both mean and std")
    if mean is not None:
        mean, std = _mean_std(mean, std, 1, "the video statistics are scalars: mean / std must hold one value each")
    T = max(lens)
    video = torch.empty(B, T, LIP_H, LIP_W, dtype=torch.float32, device=c.device)
    if T == 0 or rows == 0:                     # nothing to decode, nothing to count
        return video.zero_(), torch.LongTensor(lens)
    if c.data_ptr() % 16:
        c = c.clone()
    d = L.LipDesc(B, max(n_in), rows, T, LIP_W, LIP_H, p, q, int(bool(quantize)), float(eps))
    ws = _ws(L.lib().avvad_lip_decode_workspace(C.byref(d)), c.device)
    idx = torch.tensor([starts, n_in, n_out if n_out is not None else lens, [0] * B], dtype=torch.int32).to(c.device)
    L.check(L.lib().avvad_lip_decode(L.ptr(c), L.ptr(idx[0]), L.ptr(idx[1]), L.ptr(idx[2]) if n_out is not None else None, L.ptr(video),
                                     L.ptr(idx[3]), L.ptr(acc), L.ptr(mean), L.ptr(std), C.byref(d), L.ptr(ws), ws.numel() * 4, _stream()),
            "avvad_lip_decode")
    return video, torch.LongTensor(lens)
