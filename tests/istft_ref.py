"""The oracle of the inverse STFT tests: a float64 numpy restatement of librosa's ``istft`` (what the reference's
``packages/processing/stft.py:63-99`` calls) -- per-frame ``irfft``, periodic Hann synthesis window, overlap-add, division by
the window sum of squares where it exceeds float32 ``tiny``, ``center`` trim and ``length`` crop / zero-fill -- plus a
float32 evaluation of the same transform in the GEMM form the GPU uses, which gives the tests their error yardstick.

A spectrum is one utterance as a complex (T, F) array (frame-major, like the GPU's batched layout).

The error measure: the first and last samples divide by ``hann^2`` down to 8.9e-11 (1024 / 256), where float32 itself is off
by 8e-3, so outputs are compared through the numerator: ``E = max_s |y[s] * wss64[s] - num64[s]|`` (``weighted_error``).
Every sample is covered.  The bound is ``8 * E_cpu32``, ``E_cpu32`` being the same measure of ``istft32_gemm`` on the same
input (the factor: the MFMA's K order differs from the BLAS's; a strictly sequential float32 sum already sits at 1-2x)."""
import numpy as np

TINY32 = float(np.finfo(np.float32).tiny)      # 1.17549435e-38
FACTOR = 8.0


def hann(n_fft):
    """periodic Hann, float64 (scipy.signal.get_window('hann', n_fft, fftbins=True))"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def istft_length(T, n_fft, hop, center=False):
    if T < 1:
        return 0
    return n_fft + hop * (T - 1) - (2 * (n_fft // 2) if center else 0)


def _fit(v, start, length):
    """v[start:] cropped or zero-filled to ``length``"""
    v = v[start:]
    if length is None:
        return v
    out = np.zeros(length, dtype=v.dtype)
    n = min(length, v.size)
    out[:n] = v[:n]
    return out


def istft64(S, n_fft, hop, center=False, length=None):
    """S complex (T, F) -> (y, num, wss) float64: the output, the overlap-added numerator before the division and the
    window sum of squares, all three trimmed / cropped / zero-filled alike.  ``length=None``: librosa's default length."""
    S = np.asarray(S, dtype=np.complex128)
    T = S.shape[0]
    assert S.shape[1] == n_fft // 2 + 1 and 1 <= hop <= n_fft
    w = hann(n_fft)
    n = n_fft + hop * (T - 1)
    num, wss = np.zeros(n), np.zeros(n)
    for t in range(T):
        num[t * hop:t * hop + n_fft] += w * np.fft.irfft(S[t], n=n_fft)
        wss[t * hop:t * hop + n_fft] += w * w
    if length is None:
        length = istft_length(T, n_fft, hop, center)
    y = num.copy()
    nz = wss > TINY32
    y[nz] /= wss[nz]
    start = n_fft // 2 if center else 0
    return _fit(y, start, length), _fit(num, start, length), _fit(wss, start, length)


def inverse_basis(n_fft):
    """Winv (2F, n_fft) float64: row 2f = hann w_f/N cos(2 pi f n / N), row 2f+1 = -hann w_f/N sin(2 pi f n / N), w_f = 1
    for DC and Nyquist, else 2; the phase reduced exactly with (f n) % N."""
    F = n_fft // 2 + 1
    f, n = np.arange(F)[:, None], np.arange(n_fft)[None, :]
    ang = 2.0 * np.pi * ((f * n) % n_fft) / n_fft
    wf = np.where((f == 0) | (2 * f == n_fft), 1.0, 2.0) / n_fft
    W = np.empty((2 * F, n_fft))
    W[0::2] = hann(n_fft)[None, :] * wf * np.cos(ang)
    W[1::2] = -hann(n_fft)[None, :] * wf * np.sin(ang)
    return W


def interleave(S):
    """complex (T, F) -> real (T, 2F), (re, im) adjacent"""
    S = np.asarray(S)
    A = np.empty((S.shape[0], 2 * S.shape[1]), dtype=S.real.dtype)
    A[:, 0::2], A[:, 1::2] = S.real, S.imag
    return A


def stft32_gemm(x, n_fft, hop, pad_at_end=True, fs=16e3):
    """the forward transform in the GPU's GEMM form in float32: frames32 @ basis32 -> real (T, 2F), (re, im) adjacent"""
    x = _end_padded(np.asarray(x, dtype=np.float32), n_fft, hop, pad_at_end, fs)
    T = (x.size - n_fft) // hop + 1
    F = n_fft // 2 + 1
    k, f = np.arange(n_fft)[:, None], np.arange(F)[None, :]
    ang = 2.0 * np.pi * ((f * k) % n_fft) / n_fft
    W = np.empty((n_fft, 2 * F))
    W[:, 0::2] = hann(n_fft)[:, None] * np.cos(ang)
    W[:, 1::2] = -hann(n_fft)[:, None] * np.sin(ang)
    return np.stack([x[t * hop:t * hop + n_fft] for t in range(T)]) @ W.astype(np.float32)


def istft32_gemm(S, n_fft, hop, center=False, length=None):
    """The GEMM form in float32 on the CPU: A32 @ Winv32 (BLAS), overlap-add in float32 in ascending frame order, division
    by a float32 window sum of squares.  S complex (T, F) (rounded to complex64), or real (T, 2F) as ``stft32_gemm``
    returns it -> y float32."""
    S = np.asarray(S)
    A = (interleave(S.astype(np.complex64)) if np.iscomplexobj(S) else S).astype(np.float32)
    Y = A @ inverse_basis(n_fft).astype(np.float32)
    T = A.shape[0]
    n = n_fft + hop * (T - 1)
    w2 = (hann(n_fft) ** 2).astype(np.float32)
    num, wss = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t in range(T):
        num[t * hop:t * hop + n_fft] += Y[t]
        wss[t * hop:t * hop + n_fft] += w2
    nz = wss > np.float32(TINY32)
    num[nz] /= wss[nz]
    if length is None:
        length = istft_length(T, n_fft, hop, center)
    return _fit(num, n_fft // 2 if center else 0, length)


def weighted_error(y, num64, wss64, scale=1.0):
    """E = max_s |y[s] wss64[s] - scale num64[s]| (the weight is 1 where the output was not divided) and the two arrays"""
    w = np.where(wss64 > TINY32, wss64, 1.0)
    got = np.asarray(y, dtype=np.float64) * w
    ref = scale * np.asarray(num64, dtype=np.float64)
    return (float(np.abs(got - ref).max()) if got.size else 0.0), got, ref


def _end_padded(x, n_fft, hop, pad_at_end, fs):
    """the reference's one hop of zeros when the utterance is not a whole number of hops"""
    import math
    if pad_at_end:
        v = x.size / fs / (n_fft / fs) / (hop / n_fft)
        if math.ceil(v) != int(v):
            x = np.concatenate([x, np.zeros(hop, dtype=x.dtype)])
    return x


def stft64(x, n_fft, hop, pad_at_end=True, fs=16e3):
    """the forward transform of ``stft_pytorch(center=False)`` in float64: x (L,) -> complex (T, F)"""
    x = _end_padded(np.asarray(x, dtype=np.float64), n_fft, hop, pad_at_end, fs)
    T = (x.size - n_fft) // hop + 1
    w = hann(n_fft)
    return np.stack([np.fft.rfft(w * x[t * hop:t * hop + n_fft]) for t in range(T)])


def random_spectrum(rng, T, n_fft):
    """complex (T, F) whose inverse has about unit peak: the spectrum of unit-variance noise frames scaled to peak 1"""
    S = np.fft.rfft(rng.standard_normal((T, n_fft)), axis=1)
    S[:, 0] = S[:, 0].real + 1j * rng.standard_normal(T)          # imaginary parts the inverse must ignore
    S[:, -1] = S[:, -1].real + 1j * rng.standard_normal(T)
    return (S / np.abs(np.fft.irfft(S, n=n_fft, axis=1)).max()).astype(np.complex64)
