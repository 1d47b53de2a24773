"""Train-set statistics at a user's size (csrc/stats.hip): B = 256 utterances of 3 s, per-bin sum / sum of squares of the
log-power STFT features (1024 / 256, center=False), two routes over the same batch:

  fused    ``ops.stft_stats``: DFT GEMM, then one pass over the spectrum S into double partials; no feature tensor.
  unfused  the only route without it: ``ops.stft(mode=0)`` writes the (B, T, 513) features, then the frame mask and
           ``x.double()`` sums of ``x`` and ``x ** 2`` over batch and time in torch.

Device-event times of both (alternating, after a warm-up), the largest relative difference of their sums, and the
algorithmic bytes of the statistics pass.  Run it under ``rocprofv3 --kernel-trace --stats`` (a run of its own) for the
per-kernel times.

    python tools/mb_stats.py [--iters N] [--ragged]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-visual-vad_amd")]

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ragged", action="store_true", help="utterance lengths between half and the whole of --seconds")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mb_stats measures the GPU kernels"
    from avvad import ops
    B, L = a.B, int(a.seconds * 16000)
    g = torch.Generator().manual_seed(0)
    wave = torch.randn(B, L, generator=g) * torch.rand(B, 1, generator=g)
    lens = [L] * B
    if a.ragged:
        lens = [int(v) for v in torch.randint(L // 2, L + 1, (B,), generator=g)]
        lens[0] = L
        for b, n in enumerate(lens):
            wave[b, n:] = 0
    wave = wave.cuda()
    T = ops.n_frames(L, 1024, 256)
    F, ld = 513, 1028
    frames = torch.tensor([ops.n_frames(n, 1024, 256) for n in lens])
    mask = (torch.arange(T)[None, :] < frames[:, None]).cuda()
    nchunks = (B * T + 127) // 128
    byt = {"column_partials (read of S + partials)": B * T * ld * 4 + nchunks * 2 * F * 8,
           "add_partials": nchunks * 2 * F * 8 + 2 * 2 * F * 8,
           "unfused: feature write + two double passes read": B * T * F * 4 * 3}

    def fused():
        return ops.stft_stats(ops.stats_new(F, wave.device), wave, lens)

    def unfused():
        x = ops.stft(wave, 1024, 256, mode=0)
        xd = x.double() * mask[:, :, None]
        return torch.cat([xd.sum(dim=(0, 1)), (xd * xd).sum(dim=(0, 1)), mask.sum().double().view(1)])

    a0, b0 = fused(), unfused()
    torch.cuda.synchronize()
    rel = float(((a0 - b0).abs() / b0.abs().clamp_min(1e-300)).max())
    res = {"fused_stft_stats_ms": [], "unfused_stft_then_torch_ms": []}
    for _ in range(3):                                   # alternate the two routes: three windows each
        for name, f in (("fused_stft_stats_ms", fused), ("unfused_stft_then_torch_ms", unfused)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(round(e0.elapsed_time(e1) / a.iters, 4))
    print(json.dumps(dict(B=B, L=L, T=T, counted_frames=int(frames.sum()), max_rel_diff_of_sums=rel, algorithmic_bytes=byt, **res)))


if __name__ == "__main__":
    main()
