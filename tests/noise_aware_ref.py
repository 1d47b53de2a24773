"""float64 restatement of the reference's noise-aware masks (packages/processing/target.py noise_aware_IBM :151-202,
threshold_IBM :205-251) and of the ideal ratio mask, from spectra and the two threshold tables.

Per cell: xP = |X|^2 / p^2, nP = |N|^2 / p^2 (or a constant), speech = (xP / c_speech > nP) & (xP / c_speech > floor),
noise = (xP / c_noise < nP) | (xP / c_noise < floor); bins below low_cut - 1 and from high_cut on are 0 in the speech mask
and 1 in the noise mask; irm = xP / (xP + nP), 0 where the sum is 0.  Spectra are (..., T, F) complex arrays; a complex64
input is widened exactly, and then every operation here is one correctly rounded double operation, in the order the
kernel (csrc/target.hip noise_aware_mask) performs them, so the two agree bit for bit."""
import numpy as np


def power(S, p2=1.0):
    """(re^2 + im^2) / p2 in float64; the squares of float32 values are exact in double."""
    S = np.asarray(S)
    re, im = S.real.astype(np.float64), S.imag.astype(np.float64)
    return (re * re + im * im) / p2


def peak_sq(peak, shape):
    """peak (B,) float32 or None -> p^2 broadcast over a (B, T, F) spectrum; 1 where it is not finite and positive"""
    if peak is None:
        return 1.0
    p = np.asarray(peak, dtype=np.float32).astype(np.float64).reshape(-1)
    p2 = p * p
    p2 = np.where(np.isfinite(p2) & (p2 > 0), p2, 1.0)
    return p2.reshape((-1,) + (1,) * (len(shape) - 1))


def parts(X, N, c_speech, c_noise, low_cut=5, high_cut=500, noise_psd=10.0, peak=None):
    """-> dict: xP, nP (arrays like X), xs = xP / c_speech, xn = xP / c_noise, cut (F,) bool: the bins the cuts force"""
    X = np.asarray(X)
    p2 = peak_sq(peak, X.shape)
    xP = power(X, p2)
    nP = power(N, p2) if N is not None else np.full_like(xP, noise_psd)
    f = np.arange(X.shape[-1])
    return dict(xP=xP, nP=nP, xs=xP / np.asarray(c_speech, np.float64), xn=xP / np.asarray(c_noise, np.float64),
                cut=(f < low_cut - 1) | (f >= high_cut))


def noise_aware(X, N, c_speech, c_noise, low_cut=5, high_cut=500, floor=0.005, noise_psd=10.0, peak=None, n_frames=None):
    """-> (speech bool, noise bool, irm float32), shaped like X.  N None: nP = noise_psd (threshold_IBM).  n_frames (B,):
    frames from n_frames[b] on are zero in all three (X is (B, T, F) then)."""
    p = parts(X, N, c_speech, c_noise, low_cut, high_cut, noise_psd, peak)
    speech = (p["xs"] > p["nP"]) & (p["xs"] > floor) & ~p["cut"]
    noise = (p["xn"] < p["nP"]) | (p["xn"] < floor) | p["cut"]
    total = p["xP"] + p["nP"]
    with np.errstate(invalid="ignore", divide="ignore"):
        irm = np.where(total == 0, 0.0, p["xP"] / total).astype(np.float32)
    if n_frames is not None:
        live = np.arange(speech.shape[1])[None, :] < np.asarray(n_frames).reshape(-1, 1)
        speech, noise, irm = speech & live[..., None], noise & live[..., None], irm * live[..., None].astype(np.float32)
    return speech, noise, irm


def dft64(x, nfft=1024, hop=256, pad_at_end=True, fs=16e3, wlen_sec=64e-3, hop_percent=0.25):
    """(frames, bins) complex128 STFT of a 1-D signal: periodic Hann, no centring, the reference's one-hop end pad."""
    import math
    x = np.asarray(x, dtype=np.float64)
    if pad_at_end:
        utt = len(x) / fs
        if math.ceil(utt / wlen_sec / hop_percent) != int(utt / wlen_sec / hop_percent):
            x = np.pad(x, (0, hop))
    n = 1 + (len(x) - nfft) // hop
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft)
    frames = x[np.arange(n)[:, None] * hop + np.arange(nfft)[None, :]] * w
    return np.fft.rfft(frames, axis=1)


def bands(X, N, c_speech, c_noise, delta, floor=0.005, noise_psd=10.0):
    """Cells whose decision a DFT error of delta * max|S| per spectrum value can turn -> (speech band, noise band), bool
    like X.  With dx = delta max|X|, a power |X|^2 moves by at most e_x = 2 |X| dx + dx^2 (e_n likewise; 0 for the constant
    noise power), so a mask with table c is undecided where |xP/c - nP| <= e_x/c + e_n or |xP/c - floor| <= e_x/c."""
    X = np.asarray(X, dtype=np.complex128)
    dx = delta * np.abs(X).max()
    e_x = 2 * np.abs(X) * dx + dx * dx
    if N is None:
        nP, e_n = np.full(X.shape, noise_psd), 0.0
    else:
        N = np.asarray(N, dtype=np.complex128)
        dn = delta * np.abs(N).max()
        nP, e_n = np.abs(N) ** 2, 2 * np.abs(N) * dn + dn * dn
    xP = np.abs(X) ** 2
    out = []
    for c in (np.asarray(c_speech, np.float64), np.asarray(c_noise, np.float64)):
        out.append((np.abs(xP / c - nP) <= e_x / c + e_n) | (np.abs(xP / c - floor) <= e_x / c))
    return tuple(out)
