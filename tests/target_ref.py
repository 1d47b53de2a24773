"""float64 restatement of the reference's label functions (packages/processing/target.py), without librosa.

clean_speech_VAD (:5-56): one hop of zeros at the end when ceil(len/fs/wlen_sec/hop_percent) != int(...) (:34-40),
np.pad(n_fft//2, pad_mode) when centred (:44-45), librosa.util.frame -> 1 + (len - n_fft)//hop frames (:47),
E = sum(y^2) per frame (:54), vad = E > 10**vad_threshold * min(E) (:56).  Here E is summed in float64 (the reference
sums float32), so the two agree except where E lies within the float32 rounding of the threshold.
clean_speech_IBM (:58-70): 20 log10(|S| + eps) > max(20 log10(|S| + eps)) - ibm_threshold, over the whole (F, T) array,
here in float64.  noise_robust_clean_speech_IBM (:72-107): the IBM times the VAD, broadcast over frequency."""
import math

import numpy as np


def frames_of(y, fs=16e3, wlen_sec=50e-3, hop_percent=0.25, center=True, pad_mode="reflect", pad_at_end=True):
    """(T, n_fft) float64 frames of the end-padded, optionally centred signal (target.py:28-47)."""
    nfft = int(wlen_sec * fs)
    hop = int(hop_percent * nfft)
    y = np.asarray(y, dtype=np.float64)
    if pad_at_end:
        utt_len = len(y) / fs
        if math.ceil(utt_len / wlen_sec / hop_percent) != int(utt_len / wlen_sec / hop_percent):
            y = np.pad(y, (0, hop), mode="constant")
    if center:
        y = np.pad(y, int(nfft // 2), mode=pad_mode)
    n = 1 + (len(y) - nfft) // hop
    idx = np.arange(n)[:, None] * hop + np.arange(nfft)[None, :]
    return y[idx]


def vad_energy(y, **kw):
    """(E float64 (T,), coefficient 10**vad_threshold as a float64)."""
    thr = kw.pop("vad_threshold", 1.70)
    return (frames_of(y, **kw) ** 2).sum(axis=1), np.power(10, np.float64(thr))


def clean_speech_VAD(y, vad_threshold=1.70, **kw):
    E, c = vad_energy(y, vad_threshold=vad_threshold, **kw)
    return (E > c * E.min()).astype(np.float32)[None]


def ibm_parts(S, eps=1e-8, ibm_threshold=50):
    """(mask bool (F, T), |S| float64, max|S|, threshold magnitude (max|S| + eps) 10^(-thr/20) - eps)."""
    mag = np.abs(np.asarray(S, dtype=np.complex128))
    db = 20 * np.log10(mag + eps)
    mask = db > db.max() - ibm_threshold
    M = mag.max()
    return mask, mag, M, (M + eps) * 10.0 ** (-ibm_threshold / 20.0) - eps


def clean_speech_IBM(S, eps=1e-8, ibm_threshold=50):
    return ibm_parts(S, eps, ibm_threshold)[0].astype(np.float32)


def noise_robust_clean_speech_IBM(y, S, eps=1e-8, ibm_threshold=50, **kw):
    return clean_speech_IBM(S, eps, ibm_threshold) * clean_speech_VAD(y, **kw)
