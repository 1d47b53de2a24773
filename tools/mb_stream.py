"""Streaming inference at a user's size (avvad/stream.py, csrc/stream.hip): the benched head (2 x 1024 LSTM, y_dim 1)
on all three networks, with the W0 encoder where it applies, over a 300-frame utterance.

  stream    a session fed ``t`` frames per step: device events around the whole utterance, divided by the steps.
  prefix    what the code offered before: ``model.eval()`` re-run on the prefix so far, timed at prefix lengths
            16, 64 and 300 -- the cost of ONE decision there; divided by ``t`` it is the cost per new frame when a
            decision is taken every ``t`` frames.
  lstm      ``avvad_lstm_layer_fwd_state`` against ``avvad_lstm_layer_fwd`` on the same (B, T) shape (H = In = 1024).  The
            state call is timed the way a session runs it, with a real (zero-filled) state: T recurrent products, where
            the existing call, which starts from zero, does T - 1.  A second row times it with a NULL state, which skips
            step 0's product like the existing call: the same arithmetic.

Every shape is warmed up first; the routes alternate in one process; medians of ``--passes`` blocks with the spread
(max - min).  Run it under ``rocprofv3 --kernel-trace --stats`` (a run of its own) for the per-kernel times.

    python tools/mb_stream.py [--nets audio,video,av] [--B 1,16,64] [--t 1,4,16] [--frames 300] [--passes 3]
                              [--prefix 16,64,300] [--only stream|prefix|lstm]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-visual-vad_amd")]

import torch  # noqa: E402

W0 = dict(filter_width=2, quantization_channel=1, dilations=[2 ** i for i in range(10)] * 2, en_residual_channel=32,
          en_dilation_channel=32, en_bottleneck_width=256, en_pool_kernel_size=60, use_bias=True)
K, RF = 256, 2048


def timed(fn, passes_of):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(passes_of):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / passes_of


def summary(v):
    return dict(median_ms=round(statistics.median(v), 4), spread_ms=round(max(v) - min(v), 4))


def make_model(net):
    from packages.models.Audio_Net import DeepVAD_audio
    from packages.models.AV_Net import DeepVAD_AV
    from packages.models.Video_Net import DeepVAD_video
    torch.manual_seed(0)
    m = {"audio": lambda: DeepVAD_audio(2, 1024, 1, wavenet_params=W0), "video": lambda: DeepVAD_video(2, 1024, 1),
         "av": lambda: DeepVAD_AV(2, 1024, 1, wavenet_params=W0)}[net]()
    return m.cuda().eval()


def bench_net(net, Bs, ts, frames, prefixes, passes, only):
    from avvad import stream
    m = make_model(net)
    rows = []
    for B in Bs:
        wave = (torch.rand(B, 1, RF - 1 + frames * K, device="cuda") - 0.5) if net != "video" else None
        video = torch.randn(B, frames, 67, 67, device="cuda") if net != "audio" else None

        def run_stream(t):
            sess = stream.open(m, B, K)
            for t0 in range(0, frames, t):
                t1 = min(t0 + t, frames)
                a = wave[:, :, (0 if t0 == 0 else RF - 1 + t0 * K):RF - 1 + t1 * K].contiguous() if wave is not None else None
                v = video[:, t0:t1].contiguous() if video is not None else None
                sess.step(a, v)

        def run_prefix(p):
            with torch.no_grad():
                lens = [p] * B
                if net == "video":
                    return m(video[:, :p].contiguous(), lens)
                m.wavenet_en.en_pool_kernel_size = p
                a = wave[:, :, :RF - 1 + p * K].contiguous()
                return m(a, lens) if net == "audio" else m(a, video[:, :p].contiguous(), lens)

        routes = []
        if only in (None, "stream"):
            routes += [("stream t=%d" % t, (lambda t=t: run_stream(t)), -(-frames // t), t) for t in ts]
        if only in (None, "prefix"):
            routes += [("prefix p=%d" % p, (lambda p=p: run_prefix(p)), 1, None) for p in prefixes if p <= frames]
        for _, fn, _, _ in routes:                   # warm every shape
            fn()
        torch.cuda.synchronize()
        res = {name: [] for name, _, _, _ in routes}
        for _ in range(passes):                      # alternate the routes
            for name, fn, _, _ in routes:
                res[name].append(timed(fn, 1))
        for name, _, steps, t in routes:
            s = summary(res[name])
            row = dict(net=net, B=B, route=name, **s)
            if t is not None:
                row["per_step_ms"] = round(s["median_ms"] / steps, 4)
                row["per_new_frame_ms"] = round(s["median_ms"] / frames, 5)
            else:
                row["per_new_frame_ms_at_t"] = {str(t_): round(s["median_ms"] / t_, 4) for t_ in ts}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def bench_lstm(Bs, ts, passes, iters=20):
    from avvad import _lib as L
    h = L.lib()
    H = In = 1024
    g = torch.Generator(device="cuda").manual_seed(1)
    w_ih, w_hh = (torch.randn(4 * H, n, device="cuda", generator=g) / 32 for n in (In, H))
    b_ih, b_hh = (torch.randn(4 * H, device="cuda", generator=g) * 0.1 for _ in range(2))
    rows = []
    for B in Bs:
        for T in ts:
            x = torch.randn(B, T, In, device="cuda", generator=g)
            y = torch.empty(B, T, H, device="cuda")
            hT, cT = torch.zeros(B, H, device="cuda"), torch.zeros(B, H, device="cuda")
            lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
            d0, d1 = L.LstmDesc(B, T, In, H, lens.data_ptr(), 0), L.LstmDesc(B, T, In, H, lens.data_ptr(), 0)
            ws0 = torch.empty(h.avvad_lstm_workspace(C.byref(d0)) // 4, device="cuda")
            ws1 = torch.empty(h.avvad_lstm_state_workspace(C.byref(d1)) // 4, device="cuda")
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

            def existing():
                L.check(h.avvad_lstm_layer_fwd(L.ptr(x), L.ptr(w_ih), L.ptr(w_hh), L.ptr(b_ih), L.ptr(b_hh), L.ptr(y), C.byref(d0),
                                               L.ptr(ws0), ws0.numel() * 4, st), "avvad_lstm_layer_fwd")

            h0, c0 = torch.zeros(B, H, device="cuda"), torch.zeros(B, H, device="cuda")

            def state_call(hp, cp):
                L.check(h.avvad_lstm_layer_fwd_state(L.ptr(x), L.ptr(w_ih), L.ptr(w_hh), L.ptr(b_ih), L.ptr(b_hh), hp, cp,
                                                     L.ptr(y), L.ptr(hT), L.ptr(cT), C.byref(d1), L.ptr(ws1), ws1.numel() * 4, st),
                        "avvad_lstm_layer_fwd_state")

            def state():            # what a session runs: a real (here zero-filled) state in, another pair of buffers out
                state_call(L.ptr(h0), L.ptr(c0))

            def state_null():       # NULL state: step 0 skips the W_hh product, the work avvad_lstm_layer_fwd does
                state_call(None, None)
            existing(), state(), state_null()
            torch.cuda.synchronize()
            res = {"existing": [], "state": [], "state_null": []}
            for _ in range(passes):
                res["existing"].append(timed(existing, iters))
                res["state"].append(timed(state, iters))
                res["state_null"].append(timed(state_null, iters))
            e, s, n = summary(res["existing"]), summary(res["state"]), summary(res["state_null"])
            row = dict(lstm_layer=dict(B=B, T=T, H=H, In=In), avvad_lstm_layer_fwd=e, avvad_lstm_layer_fwd_state=s,
                       avvad_lstm_layer_fwd_state_null_state=n,
                       state_over_existing=round(s["median_ms"] / e["median_ms"], 3),
                       null_state_over_existing=round(n["median_ms"] / e["median_ms"], 3),
                       recurrent_steps=dict(existing=T - 1, state=T, null_state=T - 1),
                       w_hh_bytes_per_step=4 * H * H * 4, weight_bytes_per_step=4 * H * (In + H) * 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ints = lambda s: [int(v) for v in s.split(",") if v]
    ap.add_argument("--nets", default="audio,video,av")
    ap.add_argument("--B", type=ints, default=[1, 16, 64])
    ap.add_argument("--t", type=ints, default=[1, 4, 16])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--prefix", type=ints, default=[16, 64, 300])
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--only", choices=("stream", "prefix", "lstm"), default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mb_stream measures the GPU kernels"
    out = {}
    if a.only in (None, "lstm"):
        out["lstm"] = bench_lstm(a.B, a.t, a.passes)
    if a.only != "lstm":
        for net in [n for n in a.nets.split(",") if n]:
            out[net] = bench_net(net, a.B, a.t, a.frames, a.prefix, a.passes, a.only)
    print(json.dumps(dict(frames=a.frames, passes=a.passes, results=out)))


if __name__ == "__main__":
    main()
