"""Float64 restatement of the train-set standardisation statistics (the reference's scripts/create_audio_train_files.py:
196-214, 340-392): per-bin n, sum and sum of squares of the log-power spectrogram over every frame of the set,
``mean = sum / n``, ``std = sqrt((sumsq - n mean^2) / (n - 1))`` -- plus the reference's literal float32 accumulation, for
the CPU comparison of the two.  Test infrastructure only."""
import math
import os

import numpy as np

from conftest import GOLDEN

N_FFT, HOP, FS, EPS = 1024, 256, 16e3, 1e-8


def utterances():
    """The three fixture utterances as float32 waveforms (int16 / 32768, not yet peak-normalised): noisy sa1, clean sa1 and
    the first 30000 samples of the noisy one -- 185 + 185 + 115 = 485 frames, three lengths, so every batch is ragged."""
    noisy = np.load(os.path.join(GOLDEN, "utt_sa1.npz"))["samples"].astype(np.float32) / 32768.0
    clean = np.load(os.path.join(GOLDEN, "utt_sa1_clean.npz"))["samples"].astype(np.float32) / 32768.0
    return [noisy, clean, noisy[:30000].copy()]


def end_padded(x):
    """stft_pytorch's end pad (packages/processing/stft.py:134-139), the rule of ``ops.n_frames``."""
    v = len(x) / FS / (N_FFT / FS) / (HOP / N_FFT)
    return np.pad(x, (0, HOP)) if math.ceil(v) != int(v) else x


def features64(x, normalise=True):
    """(513, T) float64 log-power features of one utterance: x / max|x|, end pad, framed float64 DFT, log(|S|^2 + eps)."""
    from oracle import frontend
    x = np.asarray(x, dtype=np.float64)
    if normalise:
        x = x / np.max(np.abs(x))
    S = frontend.stft_naive(end_padded(x), N_FFT, HOP)
    return np.log(S.real ** 2 + S.imag ** 2 + EPS)


def accumulate(feats, dtype=np.float64):
    """[sum (F), sumsq (F), count] over a list of (F, T_i) feature arrays, the accumulator layout of ``ops.stats_new``."""
    F = feats[0].shape[0]
    acc = np.zeros(2 * F + 1, dtype)
    for x in feats:
        x = x.astype(dtype)
        acc[:F] += x.sum(axis=-1)
        acc[F:2 * F] += (x ** 2).sum(axis=-1)
        acc[2 * F] += x.shape[-1]
    return acc


def finalize(acc):
    """(mean, std) by the reference's formula, in the accumulator's precision."""
    F = (len(acc) - 1) // 2
    n = acc[2 * F]
    mean = acc[:F] / n
    std = np.sqrt((1 / (n - 1)) * (acc[F:2 * F] - n * mean ** 2))
    return mean, std


def stats64(feats):
    return finalize(accumulate(feats))


def stats32_literal(feats):
    """The reference as written: float32 spectrograms, ``n_samples, channels_sum, channels_squared_sum = 0., 0., 0.`` then
    ``+=`` of every file's float32 ``np.sum`` (a Python float plus a float32 array stays float32), float32 division."""
    n_samples, channels_sum, channels_squared_sum = 0., 0., 0.
    for x in feats:
        x = x.astype(np.float32)
        n_samples += x.shape[-1]
        channels_sum += np.sum(x, axis=-1)
        channels_squared_sum += np.sum(x ** 2, axis=-1)
    assert channels_sum.dtype == np.float32
    mean = channels_sum / n_samples
    std = np.sqrt((1 / (n_samples - 1)) * (channels_squared_sum - n_samples * mean ** 2))
    return mean, std
