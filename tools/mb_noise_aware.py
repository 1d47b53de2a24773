"""The noise-aware masks at a training batch's size (csrc/target.hip): B = 16 rows of L = 48 000 float32 samples
(185 frames of 513 bins each), timed three ways:

  waveform        ``ops.noise_aware_targets`` with one output, as ``mix_step`` calls it: two DFT products, the mask pass,
                  and the Python around them (the tables, one packed copy of the counts, the allocations)
  mask_pass_1     the bare ``avvad_target_noise_aware_from_spectrum`` call on spectra, tables and counts that are already
                  on the GPU, one output (the speech mask)
  mask_pass_3     the same with all three outputs

Device-event times over alternating windows after a warm-up; per route the median of the windows and their spread.
``bytes`` is the pass's compulsory traffic: 16 bytes read per cell (one float2 of each spectrum) and 4 bytes written per
cell and output; the two tables (16 F bytes) are left out.  At this size (30 .. 43 MB) the spectra stay in the 256 MB
Infinity Cache between calls, so the rate the bytes imply is printed next to HBM's 8.0 TB/s for scale and is not an HBM
rate.  Run it under ``rocprofv3 --kernel-trace --stats`` (a run of its own) for the per-kernel times.

    python tools/mb_noise_aware.py [--iters N] [--windows N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-visual-vad_amd")]

import torch  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, the MI355X's specified HBM3E rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--L", type=int, default=48000)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mb_noise_aware measures the GPU kernels"
    assert a.windows >= 3
    import numpy as np
    from avvad import _lib as L, ops
    dev = torch.device("cuda", 0)
    B, Ls = a.B, a.L
    g = torch.Generator().manual_seed(2)
    speech = (torch.randn(B, Ls, generator=g) * torch.rand(B, 1, generator=g)).to(dev)
    noise = (torch.randn(B, Ls, generator=g) * 0.3).to(dev)
    lens = [Ls] * B
    peak = (speech + noise).abs().amax(dim=1)
    X, N = ops.stft_complex(speech), ops.stft_complex(noise)
    T, F = X.shape[1], X.shape[2]
    tables = torch.from_numpy(np.stack(ops.noise_aware_tables(F))).to(dev)
    cnt = torch.full((B,), T, dtype=torch.int32, device=dev)
    outs = [torch.empty(B, T, F, device=dev) for _ in range(3)]
    st = X.stride()
    stream = ops._stream()

    def waveform():
        return ops.noise_aware_targets(speech, noise, lens, peak=peak, outputs=("speech",))

    def bare(n_out):
        ptrs = [L.ptr(t) for t in outs[:n_out]] + [None] * (3 - n_out)
        L.check(L.lib().avvad_target_noise_aware_from_spectrum(
            L.ptr(X), st[0], st[1], st[2], L.ptr(N), st[0], st[1], st[2], L.ptr(cnt), L.ptr(peak), L.ptr(tables[0]), L.ptr(tables[1]),
            5, 500, 0.005, 10.0, *ptrs, B, T, F, stream), "avvad_target_noise_aware_from_spectrum")
    routes = {"waveform": waveform, "mask_pass_1": lambda: bare(1), "mask_pass_3": lambda: bare(3)}
    for f in routes.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in routes}
    for _ in range(a.windows):                               # alternate the routes: one window each per round
        for name, f in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) / a.iters * 1e3)
    cells = B * T * F
    row = dict(B=B, L=Ls, T=T, F=F, cells=cells)
    for name, v in us.items():
        row[name] = dict(median_us=round(statistics.median(v), 2), spread_us=round(max(v) - min(v), 2))
    for n_out in (1, 3):
        byt = cells * (16 + 4 * n_out)
        rate = byt / (row["mask_pass_%d" % n_out]["median_us"] * 1e-6)
        row["mask_pass_%d" % n_out].update(bytes=byt, tb_per_s=round(rate / 1e12, 3), of_hbm_peak=round(rate / HBM_PEAK, 3))
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(windows=a.windows, iters=a.iters, result=row), f, indent=1)


if __name__ == "__main__":
    main()
