"""STOI / ESTOI at a user's size (csrc/stoi.hip): ``ops.stoi(clean, noisy, both=True)`` on a batch of B copies of the
committed 48 100-sample utterance pair (tests/golden/utt_sa1_clean.npz / utt_sa1.npz, 16 kHz), against the baseline that is
not the code under test:

  host   what a user does without the kernels: the waveforms are copied to the host and the float64 restatement of the
         definition (tests/stoi_ref.py) runs there, utterance by utterance (host clock around the copies and the arithmetic)

Device-event times of the GPU route over windows of ``iters`` calls after a warm-up, the host route by the host clock, and
the largest difference of the scores.  The batch is 6 MB and cache-resident, as a batch that was just resynthesised is.
Run it under ``rocprofv3 --kernel-trace --stats`` (a run of its own) for the per-kernel times.

    python tools/mb_stoi.py [--batch B] [--iters N] [--windows N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-visual-vad_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def host(clean, noisy):
    import stoi_ref
    x, y = clean.cpu().numpy(), noisy.cpu().numpy()
    out = np.empty((x.shape[0], 2))
    for b in range(x.shape[0]):
        r = stoi_ref.score(x[b], y[b], 16000)
        out[b] = r["stoi"], r["estoi"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mb_stoi measures the GPU kernels"
    import stoi_ref
    from avvad import ops
    x, y = stoi_ref.committed_pair()
    clean = torch.from_numpy(x).cuda().repeat(a.batch, 1)
    noisy = torch.from_numpy(y).cuda().repeat(a.batch, 1)
    for _ in range(3):
        d = ops.stoi(clean, noisy, both=True)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            ops.stoi(clean, noisy, both=True)
        e1.record()
        torch.cuda.synchronize()
        ms.append(round(e0.elapsed_time(e1) / a.iters, 5))
    host_ms = []
    for _ in range(a.windows):
        t0 = time.perf_counter()
        h = host(clean, noisy)
        host_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    print(json.dumps(dict(B=a.batch, L=int(clean.shape[1]), iters=a.iters, kernel_ms=ms, host_ms=host_ms,
                          stoi=float(d[0, 0]), estoi=float(d[0, 1]),
                          max_diff_kernel_vs_host=float(np.abs(d.cpu().numpy() - h).max()))), flush=True)


if __name__ == "__main__":
    main()
