"""The SI-SDR training path at a user's size (csrc/istft.hip, csrc/scores.hip): B = 16 utterances of 3 s at 16 kHz, Hann
1024 / hop 256, logits of a 513-bin mask model (mask_mode 2).

  resynth       ``ops.resynth`` without a graph: the forward resynthesis alone -- the yardstick;
  resynth_grad  the same call with logits that require a gradient (the graph node is the only difference);
  loss          ``ops.si_sdr_loss`` of the resynthesised waves against the clean ones, skips n_fft - hop: the sums, the
                coefficients and the gradient in the estimate, one call;
  backward      ``loss.backward()`` down to dlogits: the loss gradient scaled, then avvad_resynth_bwd -- the wave's
                transform again, q, q's transform, the epilogue pass: two forward-size GEMMs and three elementwise passes;
  step          the three together.

Device-event times (alternating, three blocks each after a warm-up, medians reported) and the ratios to the forward
resynthesis.  Run it under ``rocprofv3 --kernel-trace --stats`` (a run of its own) for the per-kernel times.

    python tools/mb_sisdr_train.py [--B 16] [--seconds 3] [--iters 20]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-visual-vad_amd")]

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mb_sisdr_train measures the GPU kernels"
    from avvad import ops
    n_fft, hop = 1024, 256
    B, Ls = a.B, int(a.seconds * 16000)
    skip = n_fft - hop
    g = torch.Generator().manual_seed(0)
    clean = (torch.randn(B, Ls, generator=g) * 0.1).cuda()
    noisy = clean + (torch.randn(B, Ls, generator=g) * 0.05).cuda()
    T = ops.n_frames(Ls, n_fft, hop)
    F = n_fft // 2 + 1
    logits = torch.randn(B, T, F, generator=g).cuda()
    leaf = logits.clone().requires_grad_(True)
    est = ops.resynth(noisy, logits, mask_mode=2, n_fft=n_fft, hop=hop)
    est_leaf = est.clone().requires_grad_(True)

    def step():
        leaf.grad = None
        ops.si_sdr_loss(ops.resynth(noisy, leaf, mask_mode=2, n_fft=n_fft, hop=hop), clean, None, skip, skip).backward()

    # the backward alone: graphs built outside the timed region, one per timed call
    graphs = []

    def build_graphs(n):
        del graphs[:]
        for _ in range(n):
            graphs.append(ops.si_sdr_loss(ops.resynth(noisy, leaf, mask_mode=2, n_fft=n_fft, hop=hop), clean, None, skip, skip))

    def backward():
        leaf.grad = None
        graphs.pop().backward()
    routes = [("resynth_ms", lambda: ops.resynth(noisy, logits, mask_mode=2, n_fft=n_fft, hop=hop), None),
              ("resynth_grad_ms", lambda: ops.resynth(noisy, leaf, mask_mode=2, n_fft=n_fft, hop=hop), None),
              ("loss_ms", lambda: ops.si_sdr_loss(est_leaf, clean, None, skip, skip), None),
              ("backward_ms", backward, build_graphs),
              ("step_ms", step, None)]
    for _, f, prep in routes:                            # warm-up
        if prep:
            prep(1)
        f()
    torch.cuda.synchronize()
    res = {name: [] for name, _, _ in routes}
    for _ in range(3):                                   # alternate the routes: three blocks each
        for name, f, prep in routes:
            if prep:
                prep(a.iters)
                torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(round(e0.elapsed_time(e1) / a.iters, 4))
    med = {name.replace("_ms", "_median_ms"): statistics.median(v) for name, v in res.items()}
    ratio = {k + "_over_resynth": round(med[k + "_median_ms"] / med["resynth_median_ms"], 3) for k in ("loss", "backward", "step")}
    ld = (2 * F + 3) // 4 * 4
    info = dict(B=B, samples=Ls, frames=T, mask_mode=2, gemm_gflop_one_direction=round(2.0 * B * T * n_fft * ld / 1e9, 3))
    print(json.dumps(dict(**info, **res, **med, **ratio)))


if __name__ == "__main__":
    main()
