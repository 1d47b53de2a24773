"""The streaming masked inverse STFT at a user's size (csrc/istft_stream.hip, avvad/stream.py: Session.step_enhance).

  call      one ``ops.istft_stream`` call that takes ``t`` new frames per row mid-stream (sigmoid mask from logits, the
            peak as scale, spare state swapped) and emits ``t * 256`` samples, against the one-shot route to the same
            samples: ``ops.istft`` on the ``t + n_fft / hop - 1`` frames that cover them.
  session   ``Session.step_enhance`` per packet of 256 samples against ``Session.step_wave`` on the same model (h32,
            513 outputs) over a 300-frame utterance -- the difference is the price of the samples -- timed around frame 16
            and around frame 300: a streaming session must cost the same at both.
  prefix    the only route to the same samples without the streaming inverse: ``ops.resynth`` over the whole prefix of the
            utterance, at frame 16 and at frame 300 (the model's own re-run over the prefix is NOT included: a lower bound).

Device events; every shape is warmed up first; the routes alternate in one process; medians of ``--passes`` blocks of
``--iters`` calls with the spread (max - min).

    python tools/mb_istft_stream.py [--B 1,8,64] [--t 1,4,16] [--passes 5] [--iters 50] [--only call|session|prefix]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-visual-vad_amd")]

import torch  # noqa: E402

N_FFT, HOP, F = 1024, 256, 513


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # microseconds


def summary(v):
    return dict(median_us=round(statistics.median(v), 2), spread_us=round(max(v) - min(v), 2))


def alternate(routes, passes, iters):
    for fn in routes.values():                        # warm every shape
        fn()
    torch.cuda.synchronize()
    res = {k: [] for k in routes}
    for _ in range(passes):
        for k, fn in routes.items():
            res[k].append(timed(fn, iters))
    return {k: summary(v) for k, v in res.items()}


def bench_call(Bs, ts, passes, iters):
    from avvad import ops
    from avvad.stream import OlaClock
    basis = ops.istft_stream_basis(N_FFT, "cuda")
    cover = N_FFT // HOP - 1
    rows = []
    for B in Bs:
        for t in ts:
            spec = torch.randn(B, t + cover, F, 2, device="cuda")
            logit = torch.randn(B, t + cover, F, device="cuda")
            new_spec, new_logit = spec[:, cover:].contiguous(), logit[:, cover:].contiguous()
            scale = torch.rand(B, device="cuda") + 0.5
            clock = OlaClock(B, N_FFT, HOP)
            box = [ops.istft_stream_state(B, N_FFT, "cuda"), ops.istft_stream_state(B, N_FFT, "cuda")]
            ops.istft_stream(spec[:, :cover].contiguous(), [cover] * B, clock, box[0], basis, logit[:, :cover].contiguous(), 2,
                             scale, None, box[1])    # mid-stream: the state holds the sums of three frames
            box.reverse()

            def new():
                y, n = ops.istft_stream(new_spec, [t] * B, clock, box[0], basis, new_logit, 2, scale, None, box[1])
                box.reverse()
                return y

            def window():
                return ops.istft(spec, N_FFT, HOP, mask=logit, mask_mode=2, scale=scale)
            assert new().shape == (B, t * HOP) and window().shape == (B, N_FFT + (t + cover - 1) * HOP)
            r = alternate({"istft_stream": new, "istft_on_the_window": window}, passes, iters)
            row = dict(B=B, t=t, M=B * t, **r,
                       new_over_window=round(r["istft_stream"]["median_us"] / r["istft_on_the_window"]["median_us"], 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def bench_session(Bs, passes, frames=300, at=(16, 300), width=8):
    """per packet of HOP samples (one new frame), averaged over the ``width`` packets that end at frame ``at``"""
    from avvad import stream
    from packages.models.Audio_Net import DeepVAD_audio
    torch.manual_seed(0)
    m = DeepVAD_audio(2, 32, F).cuda().eval()
    rows = []
    for B in Bs:
        wave = torch.rand(B, N_FFT - HOP + frames * HOP, device="cuda") - 0.5
        packets = [wave[:, :N_FFT - HOP].contiguous()] + \
                  [wave[:, N_FFT - HOP + k * HOP:N_FFT + k * HOP].contiguous() for k in range(frames)]

        def run(enhance):
            """-> {frame: microseconds per packet around it}"""
            s = stream.open(m, B)
            step = (lambda w: s.step_enhance(w, hard=False)) if enhance else s.step_wave
            marks = {}
            for k, w in enumerate(packets):                         # packet k > 0 completes frame k
                for a in at:
                    if k == a - width + 1:
                        marks[a] = [torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)]
                        marks[a][0].record()
                step(w)
                for a in at:
                    if k == a:
                        marks[a][1].record()
            torch.cuda.synchronize()
            return {a: e[0].elapsed_time(e[1]) / width * 1e3 for a, e in marks.items()}
        run(True), run(False)                                       # warm both routes
        res = {(route, a): [] for route in ("step_enhance", "step_wave") for a in at}
        for _ in range(passes):
            for route in ("step_enhance", "step_wave"):
                for a, us in run(route == "step_enhance").items():
                    res[(route, a)].append(us)
        row = dict(model="h32 y513", B=B, packet=HOP)
        for (route, a), v in res.items():
            row["%s_at_frame_%d" % (route, a)] = summary(v)
        for a in at:
            row["samples_cost_us_at_frame_%d" % a] = round(row["step_enhance_at_frame_%d" % a]["median_us"] -
                                                           row["step_wave_at_frame_%d" % a]["median_us"], 2)
        lo, hi = row["step_enhance_at_frame_%d" % at[0]], row["step_enhance_at_frame_%d" % at[-1]]
        row["frame_%d_within_spread_of_frame_%d" % (at[-1], at[0])] = bool(
            abs(hi["median_us"] - lo["median_us"]) <= max(lo["spread_us"], hi["spread_us"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def bench_prefix(Bs, passes, iters, at=(16, 300)):
    from avvad import ops
    rows = []
    for B in Bs:
        routes = {}
        for a in at:
            wave = torch.rand(B, N_FFT + (a - 1) * HOP, device="cuda") - 0.5
            logit = torch.randn(B, a, F, device="cuda")
            scale = torch.rand(B, device="cuda") + 0.5
            assert ops.n_frames(wave.shape[1], N_FFT, HOP) == a
            routes["resynth_prefix_at_frame_%d" % a] = (lambda w=wave, z=logit, s=scale: ops.resynth(w, z, mask_mode=2, scale=s))
        r = alternate(routes, passes, iters)
        row = dict(B=B, **r)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ints = lambda s: [int(v) for v in s.split(",") if v]      # noqa: E731
    ap.add_argument("--B", type=ints, default=[1, 8, 64])
    ap.add_argument("--t", type=ints, default=[1, 4, 16])
    ap.add_argument("--session-B", type=ints, default=[1, 8])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", choices=("call", "session", "prefix"), default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mb_istft_stream measures the GPU kernels"
    out = {}
    if a.only in (None, "call"):
        out["call"] = bench_call(a.B, a.t, a.passes, a.iters)
    if a.only in (None, "session"):
        out["session"] = bench_session(a.session_B, a.passes)
    if a.only in (None, "prefix"):
        out["prefix"] = bench_prefix(a.session_B, a.passes, a.iters)
    print(json.dumps(dict(passes=a.passes, iters=a.iters, results=out)))


if __name__ == "__main__":
    main()
