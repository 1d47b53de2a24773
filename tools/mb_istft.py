"""The masked inverse STFT at a user's size (csrc/istft.hip): B = 16 utterances of 3 s at 16 kHz, Hann 1024 / hop 256.

  resynth  ``ops.resynth``: forward DFT -> mask applied while the spectrum is loaded -> inverse DFT GEMM -> overlap-add,
           the spectrum never leaving the workspace;
  istft    ``ops.istft`` on a given (B,T,F,2) spectrum with the same mask: the inverse GEMM and the overlap-add alone;
  stft     ``ops.stft(mode=1)`` at the same shape: the forward transform.  The inverse GEMM has the same flop count
           (M = B T, K x N = 1024 x 1028 against 1028 x 1024), so this is the yardstick.

Device-event times (alternating, three blocks each after a warm-up, medians reported), the ratios to the forward
transform and the share of the fp32 MFMA peak (157.3 TFLOP/s) of each GEMM-bound route by algorithmic FLOPs.  Run it under
``rocprofv3 --kernel-trace --stats`` (a run of its own) for the per-kernel times.

    python tools/mb_istft.py [--B 16] [--seconds 3] [--iters 20] [--mode 1] [--only resynth|istft|stft]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-visual-vad_amd")]

import torch  # noqa: E402

FP32_PEAK = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--mode", type=int, default=1, choices=(0, 1, 2, 3), help="mask_mode of the two inverse routes")
    ap.add_argument("--only", choices=("resynth", "istft", "stft"), default=None, help="time one route only (profiling runs)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mb_istft measures the GPU kernels"
    from avvad import ops
    n_fft, hop = 1024, 256
    B, Ls = a.B, int(a.seconds * 16000)
    g = torch.Generator().manual_seed(0)
    wave = (torch.randn(B, Ls, generator=g) * 0.1).cuda()
    T = ops.n_frames(Ls, n_fft, hop)
    F = n_fft // 2 + 1
    mask = None if a.mode == 0 else (torch.rand(B, T, F, generator=g) if a.mode == 1 else torch.randn(B, T, F, generator=g)).cuda()
    spec = ops.stft_complex(wave, n_fft, hop)
    routes = [("resynth_ms", lambda: ops.resynth(wave, mask, mask_mode=a.mode, n_fft=n_fft, hop=hop)),
              ("istft_ms", lambda: ops.istft(spec, n_fft, hop, mask=mask, mask_mode=a.mode, length=Ls)),
              ("stft_ms", lambda: ops.stft(wave, n_fft, hop, mode=1))]
    if a.only:
        routes = [r for r in routes if r[0].startswith(a.only)]
    for _, f in routes:                                  # warm-up
        f()
    torch.cuda.synchronize()
    res = {name: [] for name, _ in routes}
    for _ in range(3):                                   # alternate the routes: three blocks each
        for name, f in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(round(e0.elapsed_time(e1) / a.iters, 4))
    med = {name.replace("_ms", "_median_ms"): statistics.median(v) for name, v in res.items()}
    ld = (2 * F + 3) // 4 * 4
    gemm_flop = 2.0 * B * T * n_fft * ld                 # one direction
    flops = {"resynth": 2 * gemm_flop, "istft": gemm_flop, "stft": gemm_flop}
    info = dict(B=B, samples=Ls, frames=T, mask_mode=a.mode, gemm_gflop_one_direction=round(gemm_flop / 1e9, 3))
    share = {k + "_share_of_fp32_peak": round(flops[k] / (med[k + "_median_ms"] * 1e-3) / FP32_PEAK, 4)
             for k in flops if k + "_median_ms" in med}
    ratio = {}
    if "stft_median_ms" in med:
        ratio = {k + "_over_stft": round(med[k + "_median_ms"] / med["stft_median_ms"], 3)
                 for k in ("resynth", "istft") if k + "_median_ms" in med}
    print(json.dumps(dict(**info, **res, **med, **ratio, **share)))


if __name__ == "__main__":
    main()
