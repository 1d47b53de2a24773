"""float64 restatement (numpy only) of the video front-end: lip-region DCT coefficients -> 67x67 crops at the STFT's frame
rate.  The specification of csrc/lip.hip and the yardstick of tests/test_lip_cpu.py / test_lip_gpu.py.

Reference: scripts/create_video_train_files_upsampled.py:105-173 (``process_write_video``) --
  A[n]   = idct(idct(X_n).T).T            scipy's unnormalised type-2 idct, X_n = coef[n].reshape(W, H)
  V[n]   = (A[n] - A.min()) / (A.max(axis=(-2, -1)) - A.min(axis=(-2, -1))).max() * 255
  out[n] = np.rot90(V[n], 3)
  frame writer: uint8 conversion (clip, truncate), then ffmpeg's ``fps`` filter to 62.5 frames/s and an x264 round trip.
The codec round trip is NOT modelled.  The ``fps`` filter is read as: output frame k shows input frame i for
s(i) <= k < s(i+1), s(i) = round_half_away(i p / q), p / q = fs / (hop fps_in).  A range of 0 (constant frames) divides by
zero in the reference; here such an utterance is written as 0."""
from fractions import Fraction

import numpy as np

W = H = 67


def dct_matrix(n=W):
    """C[k][m] = 1 for m == 0, 2 cos(pi (2k+1) m / (2n)) otherwise: ``idct(x)[k] = sum_m C[k][m] x[m]``."""
    k = np.arange(n, dtype=np.float64)[:, None]
    m = np.arange(n, dtype=np.float64)[None, :]
    C = 2.0 * np.cos(np.pi * (2.0 * k + 1.0) * m / (2.0 * n))
    C[:, 0] = 1.0
    return C


def idct2(coef):
    """(N, W*H) -> A (N, W, H): C X C^T per frame."""
    X = np.asarray(coef, np.float64).reshape(-1, W, H)
    C = dct_matrix()
    return np.einsum("ia,nab,jb->nij", C, X, C, optimize=True)


def normalise(A):
    """(A - global min) / (largest per-frame range) * 255; a range of 0 gives zeros (the stated difference)."""
    if A.shape[0] == 0:
        return A.copy()
    R = (A.max(axis=(-2, -1)) - A.min(axis=(-2, -1))).max()
    if R == 0:
        return np.zeros_like(A)
    return (A - A.min()) / R * 255.0


def rot90_3(V):
    """np.rot90(V[n], 3) written out: out[i][j] = V[H-1-j][i]."""
    return np.ascontiguousarray(np.transpose(V[:, ::-1, :], (0, 2, 1)))


def quantise(x):
    """the frame writer's uint8 conversion of a float: clip to [0, 255], round towards zero"""
    return np.trunc(np.clip(x, 0.0, 255.0))


def rate(fs=16000, hop=256, fps_in=30):
    r = Fraction(fs) / (Fraction(hop) * Fraction(fps_in))
    return r.numerator, r.denominator


def frame_starts(N, fs=16000, hop=256, fps_in=30):
    p, q = rate(fs, hop, fps_in)
    return [(2 * i * p + q) // (2 * q) for i in range(N + 1)]


def frame_map(N, fs=16000, hop=256, fps_in=30):
    """input frame shown by each of the s(N) output frames"""
    s = frame_starts(N, fs, hop, fps_in)
    return np.repeat(np.arange(N), np.diff(s)).astype(np.int64)


def frames(coef, quantize=True):
    """(N, W*H) -> the N decoded frames (N, 67, 67) before the rate conversion, float64"""
    out = rot90_3(normalise(idct2(coef)))
    return quantise(out) if quantize else out


def decode(coef, n_out=None, quantize=True, fs=16000, hop=256, fps_in=30):
    """One utterance: (N, W*H) -> (T, 67, 67) float64, T = min(s(N), n_out)."""
    f = frames(coef, quantize)
    idx = frame_map(f.shape[0], fs, hop, fps_in)
    if n_out is not None:
        idx = idx[:max(int(n_out), 0)]
    return f[idx]


def synthetic_coef(N, seed=0, scale=37.0, noise=0.02):
    """Coefficients of smooth moving images plus noise: the forward transform (the inverse of ``idct2``) of a drifting
    blob on a gradient, arbitrarily scaled -- (N, W*H) float32, as a caller would hand them over."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:W, 0:H].astype(np.float64)
    t = np.arange(N, dtype=np.float64)[:, None, None]
    cx, cy = 33 + 12 * np.sin(0.21 * t + seed), 30 + 9 * np.cos(0.13 * t)
    img = np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * (7 + 3 * np.sin(0.4 * t)) ** 2)) + 0.004 * x - 0.002 * y
    img = img * (1 + 0.3 * np.sin(0.5 * t)) + noise * rng.standard_normal((N, W, H))
    Ci = np.linalg.inv(dct_matrix())
    X = np.einsum("ia,nab,jb->nij", Ci, img, Ci, optimize=True) * scale
    return X.reshape(N, W * H).astype(np.float32)
