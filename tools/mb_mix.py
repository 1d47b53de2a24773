"""The SNR mix at training sizes (csrc/mix.hip): ``ops.mix`` with the scaled noise and the info outputs at (B, L) =
(16, 80 000) and (64, 80 000) float32 samples, rows of 60 000 .. 80 000 samples, a bank of eight clips of 1 .. 10 s,
against a baseline that is not the code under test:

  torch    the same semantics as a plain torch-on-GPU expression (an index gather of the circular read, two float64 sums
           under a length mask, the gain, an axpy and a masked write); it stands in for a parent commit, which has no
           counterpart

Both routes take the batch on the GPU and the draws on the host, as the training step has them; the kernel route's time
therefore holds its one packed host-to-device copy of the draws, the torch route's its index arithmetic.  Device-event
times over alternating windows after a warm-up of every shape; per route the median of the windows and their spread.
``kernel_only`` times the bare ``avvad_mix`` call on arguments that are already on the GPU.  ``bytes`` is what the
algorithm has to move: both passes read the speech and the noise segment (16 bytes per sample below the lengths) and the
second writes the mixture and the noise over the whole pitch (8 bytes per sample) -- at these sizes (28 .. 113 MB) all of it
stays in the 256 MB Infinity Cache between the passes and between calls, so the rate it implies is not an HBM rate.
Run it under ``rocprofv3 --kernel-trace --stats`` (a run of its own) for the per-kernel times.

    python tools/mb_mix.py [--iters N] [--windows N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-visual-vad_amd")]

import torch  # noqa: E402

SHAPES = ((16, 80000), (64, 80000))


def torch_mix(clean, lens_dev, bank, clip_dev, start_dev, ratio_dev):
    """noisy, noise, gain of the same semantics in stock torch ops (float64 sums; one rounded product, one rounded sum)"""
    B, L = clean.shape
    i = torch.arange(L, device=clean.device).unsqueeze(0)
    live = i < lens_dev.unsqueeze(1)
    cl = bank.clip_len[clip_dev].long().unsqueeze(1)
    idx = bank.clip_off[clip_dev].unsqueeze(1) + (start_dev.unsqueeze(1) + i) % cl
    n = torch.where(live, bank.data[idx], torch.zeros((), device=clean.device))
    s = torch.where(live, clean, torch.zeros((), device=clean.device))
    es, en = s.double().pow(2).sum(1), n.double().pow(2).sum(1)
    g = torch.sqrt(es / (en * ratio_dev)).float()
    g = torch.where((es > 0) & (en > 0), g, torch.zeros_like(g))
    noise = g.unsqueeze(1) * n
    return s + noise, noise, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mb_mix measures the GPU kernels"
    assert a.windows >= 3
    from avvad import _lib as L, ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    bank = ops.NoiseBank([torch.randn(16000 * k, generator=g) * 0.1 for k in (1, 2, 3, 4, 5, 6, 8, 10)], dev)
    results = []
    for B, Ls in SHAPES:
        clean = (torch.randn(B, Ls, generator=g) * 0.1).to(dev)
        lens = torch.randint(60000, Ls + 1, (B,), generator=g).tolist()
        clip = torch.randint(0, bank.K, (B,), generator=g).tolist()
        start = [int(torch.randint(0, bank.lengths[k], (1,), generator=g)) for k in clip]
        snr = (torch.rand(B, generator=g, dtype=torch.float64) * 25 - 5).tolist()
        idx = torch.tensor([lens, clip, start], dtype=torch.int32).to(dev)
        ratio = torch.tensor([ops.mix_ratio(v) for v in snr], dtype=torch.float64).to(dev)
        noisy, noise = torch.empty(B, Ls, device=dev), torch.empty(B, Ls, device=dev)
        gain, peak = torch.empty(B, device=dev), torch.empty(B, device=dev)
        energies = torch.empty(B, 2, dtype=torch.float64, device=dev)
        ws = torch.empty(L.lib().avvad_mix_workspace(B, Ls) // 4, device=dev)
        stream = ops._stream()

        def op():
            return ops.mix(clean, lens, bank, clip, start, snr, return_noise=True, return_info=True)

        def kernel_only():
            L.check(L.lib().avvad_mix(L.ptr(clean), Ls, L.ptr(idx[0]), L.ptr(bank.data), bank.data.numel(), L.ptr(bank.clip_off),
                                      L.ptr(bank.clip_len), bank.K, L.ptr(idx[1]), L.ptr(idx[2]), L.ptr(ratio), L.ptr(noisy), Ls,
                                      L.ptr(noise), Ls, L.ptr(gain), L.ptr(energies), L.ptr(peak), B, Ls, L.ptr(ws), ws.numel() * 4,
                                      stream), "avvad_mix")

        def stock():
            return torch_mix(clean, idx[0], bank, idx[1].long(), idx[2].long(), ratio)
        routes = {"ops_mix": op, "kernel_only": kernel_only, "torch": stock}
        for f in routes.values():                            # warm-up of this shape
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        y_k, z_k, info = op()
        y_t, z_t, g_t = stock()
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
        byt = 16 * sum(lens) + 8 * B * Ls
        row = dict(B=B, L=Ls, samples=sum(lens), bytes=byt)
        for name, v in us.items():
            row[name] = dict(median_us=round(statistics.median(v), 2), spread_us=round(max(v) - min(v), 2))
        row["kernel_only_gb_per_s"] = round(byt / (row["kernel_only"]["median_us"] * 1e-6) / 1e9, 1)
        row["torch_over_ops_mix"] = round(row["torch"]["median_us"] / row["ops_mix"]["median_us"], 2)
        row["max_rel_gain_diff_vs_torch"] = float(((info["gain"] - g_t).abs() / g_t).max())
        row["max_abs_noisy_diff_vs_torch"] = float((y_k - y_t).abs().max())
        print(json.dumps(row), flush=True)
        results.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(windows=a.windows, iters=a.iters, results=results), f, indent=1)


if __name__ == "__main__":
    main()
