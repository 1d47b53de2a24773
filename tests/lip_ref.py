"""float64 restatement (numpy only) of the video front-end: lip-region DCT coefficients -> 67x67 crops at the STFT's frame
rate.  The specification of csrc/lip.hip and the yardstick of tests/test_lip_cpu.py / test_lip_gpu.py.

Reference: scripts/create_video_train_files_upsampled.py:105-173 (``process_write_video``) --
  A[n]   = idct(idct(X_n).T).T            scipy's unnormalised type-2 idct, X_n = coef[n].reshape(W, H)
  V[n]   = (A[n] - A.min()) / (A.max(axis=(-2, -1)) - A.min(axis=(-2, -1))).max() * 255
  out[n] = np.rot90(V[n], 3)
  frame writer: uint8 conversion (clip, truncate), then ffmpeg's ``fps`` filter to 62.5 frames/s and an x264 round trip.
The codec round trip is NOT modelled.  The ``fps`` filter is read as: output frame k shows input frame i for
s(i) <= k < s(i+1), s(i) = round_half_away(i p / q), p / q = fs / (hop fps_in).  A range of 0 (constant frames) divides by
zero in the reference; here such an utterance is written as 0.

The second half holds the inputs and oracles of the cases past one loop trip: one-hot frames (closed form, the bound
counted rounding by rounding -- 1.368e-4 level; the float32 stand-in and the MI355X both show 2.39e-5 --, stand-in and
mutants), utterances whose extremes lie in chosen frames, mutant restatements, and the batches of the many-utterance cases."""
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


# ------------------------------------------------------------------------------------------ one-hot frames
# A coefficient frame with a single value x at (a, b) (flat index a * W + b) decodes to ONE product per pixel,
#   rot90(A, 3)[ii][j] = x C[ii][b] C[W - 1 - j][a],
# so no summation order enters and the float32 error of the kernel can be counted rounding by rounding.
TILE_EDGES = (0, 1, 15, 16, 17, 47, 48, 63, 64, 65, 66)      # first / last rows and columns of the 16-wide MFMA tiles


def onehot_pairs():
    """(a, b) of the one-hot utterance's frames: every a and every b once ((a, perm(a)), perm a bijection), all pairs of
    the tile-edge set, (33, 33) and the DC frame (0, 0) -- 189 frames, a count that is 1 mod 4, so that four copies packed
    one after the other start at rows of all four alignments."""
    pairs = [(a, (29 * a + 11) % W) for a in range(W)]           # 29 is invertible mod 67: every b once
    pairs += [(a, b) for a in TILE_EDGES for b in TILE_EDGES if (a, b) != (0, 0)]
    pairs.append((33, 33))                                       # C[33][m] = 2 cos(pi m / 2): exact zeros and +-2
    pairs.append((0, 0))
    return pairs


def onehot_amplitudes(n, scale=8.0):
    """Powers of two (the product with a table entry is then exact in float32), three sizes so that the frames' ranges
    differ and the quantised levels do not all fall on the same few values."""
    return scale * np.array([1.0, 0.5, 0.25])[np.arange(n) % 3]


def onehot_coef(scale=8.0):
    """(189, W*H) float32 coefficients of the one-hot utterance, its (a, b) pairs and amplitudes"""
    pairs = onehot_pairs()
    amp = onehot_amplitudes(len(pairs), scale)
    coef = np.zeros((len(pairs), W * H), np.float32)
    for n, (a, b) in enumerate(pairs):
        coef[n, a * W + b] = amp[n]
    return coef, pairs, amp


def onehot_frames64(pairs, amp, quantize=False):
    """float64 frames of the one-hot utterance from the closed form: one product per pixel, then ``normalise``'s formula
    (already rotated: min and range do not depend on the orientation)."""
    C = dct_matrix()
    A = np.stack([x * np.outer(C[:, b], C[::-1, a]) for (a, b), x in zip(pairs, amp)])
    out = normalise(A)
    return quantise(out) if quantize else out


U32 = 2.0 ** -24                                                 # unit roundoff of float32


def onehot_bound(pairs, amp):
    """Largest |float32 kernel - float64| a correct float32 evaluation of the one-hot utterance can show, in levels, by
    counting roundings (u = 2^-24, gamma_k = k u / (1 - k u)):

    * a pixel before the normalisation, A = x c1 c2: two table entries rounded once each from double, x c1 exact (x is a
      power of two), one rounding of the product with c2 (every other term of both 67-term sums is an exact zero):
      |dA| <= gamma_3 |A| <= gamma_3 Amax;
    * gmin is the minimum of such values: |dgmin| <= gamma_3 Amax;
    * R = max_n (hi_n - lo_n) is formed in double from such values: |dR| <= 2 gamma_3 Amax, and 255 / R is rounded to
      float32 once: relative error 2 gamma_3 Amax / R + u;
    * V = fl(fl(A - gmin) * inv): the subtract and the multiply round once each.
    |dV| <= (255 / R) 2 gamma_3 Amax + Vmax (2 gamma_3 Amax / R + 3 u), second-order terms covered by a factor
    (1 + 16 u), plus 1e-9 for the float64 side.  Amax, R and Vmax are taken from the float64 frames."""
    assert all(np.log2(x) == np.rint(np.log2(x)) for x in amp), "x c1 is exact only for powers of two"
    C = dct_matrix()
    A = np.stack([x * np.outer(C[:, b], C[::-1, a]) for (a, b), x in zip(pairs, amp)])
    Amax = np.abs(A).max()
    Rg = (A.max(axis=(-2, -1)) - A.min(axis=(-2, -1))).max()
    Vmax = (A.max() - A.min()) / Rg * 255.0
    g3 = 3 * U32 / (1 - 3 * U32)
    return ((255.0 / Rg) * 2 * g3 * Amax + Vmax * (2 * g3 * Amax / Rg + 3 * U32)) * (1 + 16 * U32) + 1e-9


def onehot_float32(coef, mutant=None):
    """numpy float32 stand-in of the kernel's formula, K padded to 68 as the MFMA steps are: Z = X^T C'^T, out = C Z
    with the float32 table, min / range / 255 / R as lip_utt forms them, subtract and multiply in float32.  The k = 67
    step multiplies the table's pad row (zero) with what follows the frame in memory.  ``mutant`` plants one mistake:
    "entry" (one table entry taken from the neighbouring index), "reverse" (the row reversal on the other operand),
    "pad" (a nonzero table pad row), "transpose" (X instead of X^T)."""
    c32 = np.asarray(coef, np.float32)
    N = c32.shape[0]
    tab = np.zeros((W + 1, W + 1), np.float32)                   # tab[a][i] = C[i][a], row / column 67 zero
    tab[:W, :W] = dct_matrix().T.astype(np.float32)
    if mutant == "entry":
        tab[66, 65] = tab[66, 64]
    if mutant == "pad":
        tab[W, :W] = 1.0
    flat = np.concatenate([c32.reshape(-1), np.zeros(W + 1, np.float32)])
    X = np.zeros((N, W + 1, W + 1), np.float32)
    X[:, :W, :W] = c32.reshape(N, W, W)
    for n in range(N):                                           # "row 67": the 67 values behind the frame
        X[n, W, :W] = flat[(n + 1) * W * W:(n + 1) * W * W + W]
    if mutant == "transpose":
        X[:, :W, :W] = np.transpose(X[:, :W, :W], (0, 2, 1))
    rev, fwd = tab[:, W - 1::-1], tab[:, :W]                     # [k][j] = C[66 - j][k], [k][i] = C[i][k]
    if mutant == "reverse":
        rev, fwd = fwd, rev
    Z = np.matmul(np.transpose(X, (0, 2, 1))[:, :W, :], rev)     # Z[bb][j] = sum_k X[k][bb] C[66 - j][k]
    out = np.matmul(fwd[:W].T, Z)                                # out[ii][j] = sum_bb C[ii][bb] Z[bb][j]
    assert out.dtype == np.float32
    lo, hi = out.min(axis=(-2, -1)), out.max(axis=(-2, -1))
    rg = (hi.astype(np.float64) - lo.astype(np.float64)).max()
    inv = np.float32(255.0 / rg) if rg > 0 else np.float32(0)
    V = (out - lo.min()) * inv
    assert V.dtype == np.float32
    return V.astype(np.float64)


# ------------------------------------------------------------------------------------------ long and many utterances
def float32_deviation(coef):
    """Largest per-pixel deviation from the float64 restatement of a numpy float32 evaluation of the same formula on the
    same input: the rule of test_lip_gpu.float32_deviation.  That one's three-operand einsum takes seconds for hundreds of
    frames; here the two 67-term sums are written out term by term (ascending index, every product and every addition
    rounded to float32), which costs milliseconds per frame and is the same arithmetic on every host, whatever its BLAS."""
    c32 = np.asarray(coef, np.float32).reshape(-1, W, H)
    C32 = dct_matrix().astype(np.float32)
    Y = np.zeros_like(c32)                                       # Y[n][i][b] = sum_a C[i][a] X[n][a][b]
    for a in range(W):
        Y += C32[None, :, a, None] * c32[:, a, None, :]
    A = np.zeros_like(c32)                                       # A[n][i][j] = sum_b Y[n][i][b] C[j][b]
    for b in range(H):
        A += Y[:, :, b, None] * C32[None, None, :, b]
    assert A.dtype == np.float32
    rng = (A.max(axis=(-2, -1)) - A.min(axis=(-2, -1))).max()
    V = (A - A.min()) / rng * np.float32(255.0)
    return float(np.abs(rot90_3(V) - frames(coef, quantize=False)).max())


def tolerance(coef):
    """4 x the float32 numpy deviation, never above 0.01 level: test_lip_gpu.tolerance's rule"""
    return min(4.0 * float32_deviation(coef), 0.01)


def shift_and_scale(coef, frame, gain=1.0, dc=0.0):
    """frame <- gain * frame + dc on every pixel (the DC coefficient adds a constant to the decoded frame)"""
    coef[frame] *= np.float32(gain)
    coef[frame, 0] += np.float32(dc)
    return coef


def extremes_in(coef, lo_frame, range_frame):
    """Moves the utterance's global minimum into ``lo_frame`` and its largest per-frame range into ``range_frame`` (two
    different frames), in place: the first is shifted down until its minimum lies a quarter of the utterance's span below
    every other, the second is scaled to 1.25 x the largest range and shifted so that its minimum lies above the old global
    one.  Every other frame keeps a strictly larger minimum and a strictly smaller range, and most levels stay inside
    0..255."""
    assert lo_frame != range_frame
    A = idct2(coef)
    lo, hi = A.min(axis=(-2, -1)), A.max(axis=(-2, -1))
    span = hi.max() - lo.min()
    shift_and_scale(coef, lo_frame, dc=lo.min() - 0.25 * span - lo[lo_frame])
    gain = 1.25 * (hi - lo).max() / (hi - lo)[range_frame]
    shift_and_scale(coef, range_frame, gain=gain, dc=lo.min() + 0.05 * span - gain * lo[range_frame])
    return coef


def decode_first_frames_only(coef, first, **kw):
    """MUTANT restatement: min and range from the first ``first`` frames alone (a frame loop that takes one trip)"""
    A = idct2(coef)
    head = A[:first]
    Rg = (head.max(axis=(-2, -1)) - head.min(axis=(-2, -1))).max()
    out = rot90_3((A - head.min()) / Rg * 255.0)
    return out[frame_map(out.shape[0], **kw)]


def decode_seen_frames_only(coef, **kw):
    """MUTANT restatement: min and range from the frames that get an output slot alone"""
    A = idct2(coef)
    seen = np.unique(frame_map(A.shape[0], **kw))
    head = A[seen]
    Rg = (head.max(axis=(-2, -1)) - head.min(axis=(-2, -1))).max()
    out = rot90_3((A - head.min()) / Rg * 255.0)
    return out[frame_map(out.shape[0], **kw)]


def dropped_frames(N, **kw):
    """input frames that get no output slot (p < q): s(i + 1) == s(i)"""
    return np.nonzero(np.diff(frame_starts(N, **kw)) == 0)[0]


def add_model(frame_sums, n_in, max_waves=None, max_lane_trips=None):
    """lip_add restated: wave w takes the utterances w, w + 16, ..., lane l their frames l, l + 64, ...  ``frame_sums``
    (sum N) are the per-frame partials in packed order.  MUTANTS: ``max_waves`` = 16 drops the utterances b >= 16 (no
    second trip of the utterance loop), ``max_lane_trips`` = 1 drops the frames i >= 64."""
    total, start = 0.0, 0
    for b, n in enumerate(n_in):
        if max_waves is None or b < max_waves:
            take = n if max_lane_trips is None else min(n, 64 * max_lane_trips)
            total += float(np.sum(frame_sums[start:start + take]))
        start += n
    return total


# ------------------------------------------------------------------------------------------ the cases (CPU and GPU tests)
ONE = dict(fs=16000, hop=160, fps_in=100)                        # p / q = 1: one output frame per input frame
LONG_N, LONG_LO, LONG_RANGE = 600, 300, 550                      # lip_utt walks frames 256 at a time: third trip ragged


def long_utterance():
    """600 frames whose global minimum lies in frame 300 and whose largest range lies in frame 550"""
    return extremes_in(synthetic_coef(LONG_N, seed=11, scale=5.0), LONG_LO, LONG_RANGE)


def stats_add_counts():
    """B = 35 frame counts within 0..130: three above 128 (a third trip of lip_add's lane loop), 64 / 65 (the edge of the
    second), zeros, and utterances b >= 16 and b >= 32 (second and third trip of its utterance loop)"""
    n = [129, 3, 0, 64, 7, 65, 1, 12, 2, 130, 5, 0, 9, 4, 17, 6, 11, 8, 129, 2, 33, 1, 0, 10, 3, 66, 5, 7, 2, 14, 4, 1, 63, 6, 128]
    assert len(n) == 35 and sum(v > 128 for v in n) == 3 and 0 in n and max(n) == 130
    return n


def batch_of(n_in, seed, scale=3.0):
    """packed coefficients of a batch: consecutive runs of one long synthetic sequence, each utterance scaled differently"""
    pool = synthetic_coef(sum(n_in), seed=seed, scale=scale)
    start = 0
    for b, n in enumerate(n_in):
        pool[start:start + n] *= np.float32(1.0 + 0.125 * (b % 5))
        start += n
    return pool


def split(packed, n_in):
    ends = np.cumsum(n_in)
    return [packed[e - n:e] for e, n in zip(ends, n_in)]


def count_counts():
    """B = 1030 > 1024 utterances of one or two frames: the second trip of lip_add's count loop, and a grid of one
    workgroup per utterance (256 / B == 0)"""
    return [1 + (b * 7 % 3 == 0) for b in range(1030)]


def ragged_counts():
    """B = 128 utterances of 9..13 frames: two workgroups per utterance, eight frames per trip, two trips, ragged ends"""
    return [9 + (5 * b + b // 7) % 5 for b in range(128)]


RATES = (25, 50, 100, 125)                                       # at hop 256: p / q = 5/2, 5/4, 5/8, 1/2 (ties at 125)


def rate_utterances(fps_in):
    """Two utterances (50 and 37 frames) for the rate ``fps_in`` at hop 256.  Where the rate drops frames (p < q), the
    global minimum and the largest range of each lie in frames that get no output slot."""
    utts = []
    for b, n in enumerate((50, 37)):
        coef = synthetic_coef(n, seed=31 + b, scale=2.0 + b)
        gone = dropped_frames(n, hop=256, fps_in=fps_in)
        if len(gone):
            assert len(gone) >= 2
            extremes_in(coef, int(gone[len(gone) // 2]), int(gone[-1]))
        utts.append(coef)
    return utts
