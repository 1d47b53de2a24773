"""The resampler at working sizes (csrc/resample.hip): ``ops.resample`` on 16 utterances of 3 s at 48 kHz (1/3, taps and
input span in LDS) and at 44.1 kHz (160/441, 8 960 taps read from global memory), and one packet stream per rate --
16 rows fed 10 ms packets through ``ops.resample_stream`` -- against a baseline that is not the code under test:

  scipy    ``scipy.signal.resample_poly`` of the same batch on the host (float64), where scipy imports; it is what a user
           without this kernel runs before the GPU path can start.  Its time holds no transfer.

Device-event times over alternating windows after a warm-up of every shape; per route the median of the windows and
their spread.  ``kernel_only`` times the bare ``avvad_resample`` call on arguments that are already on the GPU; the
streamed figure is per packet and is dominated by the launch and the one packed host-to-device copy of the counts.
``dfma`` is the number of double fma's the outputs need (terms per output times outputs), the work a roofline of this
kernel is made of: each output is one dependent chain of 21 .. 121 of them.
Run it under ``rocprofv3 --kernel-trace --stats`` (a run of its own) for the per-kernel times.

    python tools/mb_resample.py [--iters N] [--windows N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-visual-vad_amd")]

import torch  # noqa: E402

RATES = (48000, 44100)
B, SECONDS, PACKET_MS = 16, 3, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mb_resample measures the GPU kernels"
    assert a.windows >= 3
    from avvad import _lib as L, ops
    from avvad.stream import RateClock
    try:
        from scipy.signal import resample_poly
    except ImportError:
        resample_poly = None
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    results = []
    for fs in RATES:
        up, down = ops.resample_ratio(fs)
        Ls = fs * SECONDS
        x = (torch.randn(B, Ls, generator=g) * 0.1).to(dev)
        taps = ops.resample_taps_on(up, down, dev)
        Lout = ops.resample_length(Ls, up, down)
        out = torch.empty(B, Lout, device=dev)
        stream = ops._stream()
        n_pk = fs * PACKET_MS // 1000
        clock = RateClock(B, up, down)
        state = ops.resample_stream_state(B, up, down, dev)
        spare = torch.empty_like(state)
        pk = x[:, :n_pk].contiguous()

        def op():
            return ops.resample(x, fs_in=fs)

        def kernel_only():
            L.check(L.lib().avvad_resample(L.ptr(x), Ls, None, L.ptr(taps), up, down, L.ptr(out), Lout, None, B, Ls, stream),
                    "avvad_resample")

        def packet():
            return ops.resample_stream(pk, None, clock, state, taps, None, spare)
        routes = {"ops_resample": op, "kernel_only": kernel_only, "stream_packet": packet}
        for f in routes.values():                            # warm-up of this shape
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        y = op()[0]
        us = {k: [] for k in routes}
        for _ in range(a.windows):                           # alternate the routes: one window each per round
            for name, f in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    f()
                e1.record()
                torch.cuda.synchronize()
                us[name].append(e0.elapsed_time(e1) / a.iters * 1e3)
        terms = 2 * 10 * max(up, down) // up + 1
        row = dict(fs_in=fs, up=up, down=down, B=B, L=Ls, outputs=B * Lout, dfma=B * Lout * terms, packet_samples=n_pk)
        for name, v in us.items():
            row[name] = dict(median_us=round(statistics.median(v), 2), spread_us=round(max(v) - min(v), 2))
        row["kernel_only_gdfma_per_s"] = round(row["dfma"] / (row["kernel_only"]["median_us"] * 1e-6) / 1e9, 1)
        if resample_poly is not None:
            xh = x.cpu().numpy().astype("float64")
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                ref = resample_poly(xh, up, down, axis=1)
                t.append((time.perf_counter() - t0) * 1e6)
            row["scipy_host"] = dict(median_us=round(statistics.median(t), 1), spread_us=round(max(t) - min(t), 1))
            row["scipy_over_ops_resample"] = round(row["scipy_host"]["median_us"] / row["ops_resample"]["median_us"], 1)
            row["max_abs_diff_vs_scipy"] = float(abs(y.cpu().numpy().astype("float64") - ref).max())
        results.append(row)
    print(json.dumps(dict(tool="mb_resample", windows=a.windows, iters=a.iters, results=results)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(windows=a.windows, iters=a.iters, results=results), f, indent=1)


if __name__ == "__main__":
    main()
