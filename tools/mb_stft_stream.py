"""The streaming STFT front-end at a user's size (csrc/stft_stream.hip, avvad/stream.py: Session.step_wave).

  call      one ``ops.stft_stream`` call that completes ``t`` frames per row (steady state: 768 samples pending, t * 256
            new ones, statistics applied, spare state swapped) against what a caller could do before: ``ops.stft(mode=0,
            mean, std)`` on the last ``n_fft + (t - 1) * hop`` samples of each row.
  whole     whole utterances of 185 frames per row: one final ``ops.stft_stream`` call against ``ops.stft`` on the batch,
            for growing batches -- where the tile engine overtakes the basis-streaming kernel.
  session   ``Session.step_wave`` per new frame (samples in) against ``Session.step`` on ready features, for the h32 and
            the 2 x 1024 audio models over a 300-frame utterance.

Device events; every shape is warmed up first; the two routes alternate in one process; medians of ``--passes`` blocks
of ``--iters`` calls with the spread (max - min).

    python tools/mb_stft_stream.py [--B 1,8,64] [--t 1,4,16] [--passes 5] [--iters 50] [--only call|whole|session]"""
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


def stats_vectors():
    g = torch.Generator(device="cuda").manual_seed(2)
    return torch.randn(F, device="cuda", generator=g), torch.rand(F, device="cuda", generator=g) + 0.5


def bench_call(Bs, ts, passes, iters):
    from avvad import ops
    from avvad.stream import SampleClock
    mean, std = stats_vectors()
    basis = ops.stft_stream_basis(N_FFT, "cuda")
    rows = []
    for B in Bs:
        for t in ts:
            wave = torch.rand(B, N_FFT + (t - 1) * HOP, device="cuda") - 0.5
            chunk = torch.rand(B, t * HOP, device="cuda") - 0.5
            clock = SampleClock(B, N_FFT, HOP)
            box = [ops.stft_stream_state(B, N_FFT, "cuda"), ops.stft_stream_state(B, N_FFT, "cuda")]
            ops.stft_stream(wave[:, :N_FFT - HOP].contiguous(), None, clock, box[0], basis, out_state=box[1])    # 768 pending
            box.reverse()

            def new():
                _, frames = ops.stft_stream(chunk, None, clock, box[0], basis, None, mean, std, None, box[1])
                box.reverse()
                return frames

            def parent():
                return ops.stft(wave, N_FFT, HOP, mode=0, pad_at_end=False, mean=mean, std=std)
            assert new() == [t] * B and parent().shape == (B, t, F)
            r = alternate({"stft_stream": new, "stft_on_the_tail": parent}, passes, iters)
            row = dict(B=B, t=t, M=B * t, **r, new_over_parent=round(r["stft_stream"]["median_us"] / r["stft_on_the_tail"]["median_us"], 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def bench_whole(Bs, passes, iters, L=48100):
    from avvad import ops
    from avvad.stream import SampleClock
    mean, std = stats_vectors()
    basis = ops.stft_stream_basis(N_FFT, "cuda")
    T = ops.n_frames(L, N_FFT, HOP)
    rows = []
    for B in Bs:
        wave = torch.rand(B, L, device="cuda") - 0.5
        state, spare = ops.stft_stream_state(B, N_FFT, "cuda"), ops.stft_stream_state(B, N_FFT, "cuda")

        def new():
            return ops.stft_stream(wave, None, SampleClock(B, N_FFT, HOP), state, basis, None, mean, std, range(B), spare)[0]

        def parent():
            return ops.stft(wave, N_FFT, HOP, mode=0, mean=mean, std=std)
        assert new().shape == parent().shape == (B, T, F)
        r = alternate({"stft_stream": new, "stft": parent}, passes, max(iters // 5, 5))
        row = dict(B=B, M=B * T, **r, new_over_parent=round(r["stft_stream"]["median_us"] / r["stft"]["median_us"], 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def bench_session(Bs, ts, passes, frames=300):
    from avvad import ops, stream
    from packages.models.Audio_Net import DeepVAD_audio
    rows = []
    for name, H in (("h32", 32), ("2x1024", 1024)):
        torch.manual_seed(0)
        m = DeepVAD_audio(2, H, 1).cuda().eval()
        for B in Bs:
            wave = torch.rand(B, N_FFT - HOP + frames * HOP, device="cuda") - 0.5
            feats = ops.stft(wave, N_FFT, HOP, mode=0, pad_at_end=False)
            assert feats.shape[1] == frames
            for t in ts:
                def from_samples():
                    s = stream.open(m, B)
                    s.step_wave(wave[:, :N_FFT - HOP].contiguous())
                    for t0 in range(0, frames, t):
                        s.step_wave(wave[:, N_FFT - HOP + t0 * HOP:N_FFT - HOP + min(t0 + t, frames) * HOP].contiguous())

                def from_features():
                    s = stream.open(m, B)
                    for t0 in range(0, frames, t):
                        s.step(feats[:, t0:t0 + t].contiguous())
                r = alternate({"step_wave": from_samples, "step": from_features}, passes, 1)
                row = dict(model=name, B=B, t=t,
                           step_wave_us_per_new_frame=round(r["step_wave"]["median_us"] / frames, 2),
                           step_us_per_new_frame=round(r["step"]["median_us"] / frames, 2),
                           spread_us_per_new_frame=round(max(r["step_wave"]["spread_us"], r["step"]["spread_us"]) / frames, 2))
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ints = lambda s: [int(v) for v in s.split(",") if v]
    ap.add_argument("--B", type=ints, default=[1, 8, 64])
    ap.add_argument("--t", type=ints, default=[1, 4, 16])
    ap.add_argument("--whole-B", type=ints, default=[1, 2, 4, 8, 16, 32])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", choices=("call", "whole", "session"), default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mb_stft_stream measures the GPU kernels"
    out = {}
    if a.only in (None, "call"):
        out["call"] = bench_call(a.B, a.t, a.passes, a.iters)
    if a.only in (None, "whole"):
        out["whole"] = bench_whole(a.whole_B, a.passes, a.iters)
    if a.only in (None, "session"):
        out["session"] = bench_session(a.B, a.t, a.passes)
    print(json.dumps(dict(passes=a.passes, iters=a.iters, results=out)))


if __name__ == "__main__":
    main()
