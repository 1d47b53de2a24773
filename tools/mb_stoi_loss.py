"""The STOI / ESTOI training loss at the training batch (csrc/stoi.hip avvad_stoi_loss): ``ops.stoi_loss`` -- the score, the
loss and the gradient in the processed signal from one call, then ``backward`` (one scaling pass) -- on 16 rows of 5 s at
16 kHz (tests/stoi_ref.speech_pair, seeded, a third of the time gated), beside ``ops.stoi`` on the same input: what the
gradient costs over the score alone.

Device-event times over windows of ``iters`` calls after a warm-up, the two routes alternating window by window (tools/mb_stoi.py's
method), for STOI and for ESTOI.  Run it under ``rocprofv3 --kernel-trace --stats`` (a run of its own) for the per-kernel
times.

    python tools/mb_stoi_loss.py [--batch B] [--seconds S] [--iters N] [--windows N]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-visual-vad_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / iters, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mb_stoi_loss measures the GPU kernels"
    import stoi_ref
    from avvad import _lib as L, ops
    n = int(a.seconds * 16000)
    pairs = [stoi_ref.speech_pair(900 + b, n, 16000, 5.0, 0.3) for b in range(a.batch)]
    clean = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    noisy = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda().requires_grad_(True)
    out = dict(B=a.batch, L=n, iters=a.iters, workspace_mb=round(L.lib().avvad_stoi_loss_workspace(a.batch, n, 16000) / 2 ** 20, 1),
               score_workspace_mb=round(L.lib().avvad_stoi_workspace(a.batch, n, 16000) / 2 ** 20, 1))
    for name, ext in (("stoi", False), ("estoi", True)):
        def score():
            ops.stoi(clean, noisy.detach(), extended=ext)

        def loss():
            noisy.grad = None
            ops.stoi_loss(noisy, clean, extended=ext).backward()
        for _ in range(3):
            score(), loss()
        torch.cuda.synchronize()
        ms = {"score_ms": [], "loss_and_gradient_ms": []}
        for _ in range(a.windows):
            ms["score_ms"].append(timed(score, a.iters))
            ms["loss_and_gradient_ms"].append(timed(loss, a.iters))
        value, d = ops.stoi_loss(noisy, clean, extended=ext, return_scores=True)
        out[name] = dict(ms, loss=float(value.detach()), mean_score=float(d.mean()), segments=int(ops.stoi(clean, noisy.detach(), return_info=True)[1][:, 2].sum()))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
