"""Label kernels at a user's size (csrc/target.hip): B = 256 utterances of 3 s, VAD + IBM labels with the training
pipeline's framing (1024 / 256, center=False).  Run it under ``rocprofv3 --kernel-trace --stats`` for the per-kernel
times (the DFT GEMM's among them); the script itself prints the algorithmic bytes of every label kernel (what the
algorithm must read and write) and, from device events, the batch's label time next to a power spectrogram of the same
batch.

    python tools/mb_targets.py [--iters N]"""
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
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mb_targets measures the GPU kernels"
    from avvad import ops
    B, L = a.B, int(a.seconds * 16000)
    g = torch.Generator().manual_seed(0)
    wave = (torch.randn(B, L, generator=g) * torch.rand(B, 1, generator=g)).cuda()
    lens = [L] * B
    n_pad, T = ops.target_frames(L)
    F, ld = 513, 1028
    byt = {"segment_energy (VAD)": B * L * 4 + B * (T + 3) * 8,
           "vad_decide (VAD)": B * (T + 3) * 8 + B * T * 4,
           "spectrum_max (IBM)": B * T * ld * 4,
           "ibm_mask (IBM)": B * T * F * 8 + B * T * F * 4}

    def run():
        ops.speech_targets(wave, lens, "vad_labels")
        ops.speech_targets(wave, lens, "ibm_labels")

    def run_stft():
        ops.stft(wave, 1024, 256, mode=1)

    for f in (run, run_stft):
        f()
    torch.cuda.synchronize()
    res = {}
    for name, f in (("labels_vad_plus_ibm_ms", run), ("stft_power_ms", run_stft)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            f()
        e1.record()
        torch.cuda.synchronize()
        res[name] = e0.elapsed_time(e1) / a.iters
    print(json.dumps(dict(B=B, L=L, T=T, algorithmic_bytes=byt, **res)))


if __name__ == "__main__":
    main()
