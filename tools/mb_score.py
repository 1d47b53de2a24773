"""Energy ratios at a user's sizes (csrc/scores.hip): the one-shot ``ops.energy_ratios(est, clean, mixture=noisy)`` at
(B, L) = (1, 80 000), (16, 80 000) and (64, 160 000) float32 samples, against two baselines that are not the code under
test:

  torch64  the reference's formulas (packages/metrics.py:12-60) restated in float64 torch on the same GPU: the planes
           n = x - s, s_target, e_noise, e_art are written and their norms taken, batched over the rows
  host     what a user does without the kernel: the three waveforms are copied to the host and the numpy formulas run
           there, row by row (host clock around the copies and the arithmetic)

Device-event times of the two GPU routes (alternating windows, after a warm-up of every shape), the host route by the
host clock, the largest difference of the ratios in dB, and the share of the HBM peak (8 TB/s) that the compulsory
``12 * sum(len)`` bytes make of the kernel route's time.  Every call of a window takes the next of ``sets`` copies of
the inputs, 600 MB in all -- more than the 256 MB Infinity Cache -- so the signals come from HBM, as an utterance that
was just loaded does; ``--warm`` reuses one copy (cache-resident below 256 MB).  Run it under
``rocprofv3 --kernel-trace --stats`` (a run of its own) for the per-kernel times.

    python tools/mb_score.py [--iters N] [--windows N] [--warm]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-visual-vad_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = ((1, 80000), (16, 80000), (64, 160000))


def torch64(est, clean, noisy):
    e, s, x = est.double(), clean.double(), noisy.double()
    n = x - s
    dot = lambda a, b: (a * b).sum(dim=1, keepdim=True)      # noqa: E731
    s_target = dot(e, s) / dot(s, s) * s
    e_noise = dot(e, n) / dot(n, n) * n
    e_art = e - s_target - e_noise
    p = dot(s_target, s_target)
    res = e_noise + e_art
    return 10.0 * torch.log10(torch.cat([p / dot(res, res), p / dot(e_noise, e_noise), p / dot(e_art, e_art)], dim=1))


def host(est, clean, noisy):
    e, s, x = (t.cpu().numpy().astype(np.float64) for t in (est, clean, noisy))
    out = np.empty((e.shape[0], 3))
    for b in range(e.shape[0]):
        n = x[b] - s[b]
        s_target = np.dot(e[b], s[b]) / np.linalg.norm(s[b]) ** 2 * s[b]
        e_noise = np.dot(e[b], n) / np.linalg.norm(n) ** 2 * n
        e_art = e[b] - s_target - e_noise
        p = np.linalg.norm(s_target) ** 2
        out[b] = [10 * np.log10(p / np.linalg.norm(e_noise + e_art) ** 2), 10 * np.log10(p / np.linalg.norm(e_noise) ** 2),
                  10 * np.log10(p / np.linalg.norm(e_art) ** 2)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warm", action="store_true", help="one copy of the inputs for every call (cache-resident)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mb_score measures the GPU kernels"
    from avvad import ops
    for B, L in SHAPES:
        g = torch.Generator().manual_seed(B)
        clean, noise = torch.randn(B, L, generator=g), torch.randn(B, L, generator=g)
        noisy = clean + 0.3 * noise
        est = (0.7 * clean + 0.05 * noise + 0.01 * torch.randn(B, L, generator=g))
        est, clean, noisy = est.cuda(), clean.cuda(), noisy.cuda()
        sets = 1 if a.warm else min(640, int(600e6 / (12 * B * L)) + 1)
        copies = [tuple(t.clone() for t in (est, clean, noisy)) for _ in range(sets)]
        turn = [0]

        def inputs():
            turn[0] = (turn[0] + 1) % sets
            return copies[turn[0]]

        def kernel():
            e, s, x = inputs()
            return ops.energy_ratios(e, s, mixture=x)

        def planes():
            return torch64(*inputs())
        routes = {"kernel": kernel, "torch64": planes}
        for f in routes.values():                            # warm-up of this shape
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        r_k, r_t, r_h = routes["kernel"]().cpu().numpy(), routes["torch64"]().cpu().numpy(), host(est, clean, noisy)
        ms = {k: [] for k in routes}
        for _ in range(a.windows):                           # alternate the routes: one window each per round
            for name, f in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    f()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(round(e0.elapsed_time(e1) / a.iters, 5))
        host_ms = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            host(est, clean, noisy)
            host_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        byt = 12 * B * L
        best = min(ms["kernel"])
        print(json.dumps(dict(B=B, L=L, sets=sets, compulsory_bytes=byt, kernel_ms=ms["kernel"], torch64_ms=ms["torch64"], host_ms=host_ms,
                              kernel_share_of_hbm_peak=round(byt / (best * 1e-3) / HBM_PEAK, 4),
                              max_db_diff_kernel_vs_torch64=float(np.abs(r_k - r_t).max()),
                              max_db_diff_kernel_vs_host=float(np.abs(r_k - r_h).max()))), flush=True)


if __name__ == "__main__":
    main()
