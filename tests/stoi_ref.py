"""Float64 restatement of the STOI / ESTOI definition of include/avvad.h (avvad_stoi, csrc/stoi.hip), stage by stage, each
stage callable on its own; a float32 stand-in (the same stages with float32 storage where the kernels round: the resampled
samples, the overlap-added samples, the basis and the ordered float32 product of the framed DFT); the mutants that the CPU
tests use to show that the GPU bound can fail; the margin of an input (the smallest distance of a frame energy from the
keep threshold); and the inputs both test files share, with their references computed once.

A plain module: numpy only, no fixtures.

The bound.  MEASURED_STANDIN is the float32 stand-in's largest |d - d_float64| over ``CASE_NAMES`` (STOI and ESTOI), measured
on the CPU by tests/test_stoi_cpu.py, which prints the figure and holds the stand-in to GPU_BOUND / 8 = MEASURED_STANDIN
rounded up to two digits.  GPU_BOUND is 8 times that: the margin this project gives a kernel over its stand-in.  The
yardstick is always the float64 reference.

Past one trip.  ``LONG_CASE_NAMES`` is a second table of inputs, of more than 256 and more than 1024 frames, for the loops
and grids of csrc/stoi.hip that the 15 inputs above leave at one trip; ``LONG_MUTANTS`` restates how a kept-frame pass goes
wrong there.  tests/test_stoi_long_cpu.py holds their conditions and measures the stand-in over them (it stays within
MEASURED_STANDIN, so they keep GPU_BOUND); ``check_scores`` is what every GPU test asserts of a case's result.
"""
import functools
import os

import numpy as np

FS = 10000
N_FRAME, HOP, NFFT = 256, 128, 512
NUM_BANDS, MIN_FREQ = 15, 150.0
N_SEG = 30
BETA_DB = 15.0
DYN_RANGE = 40.0
EPS = 2.0 ** -52
DEGENERATE = 1e-5
F0, F1 = 7, 219                       # bins the bands need
EDGES = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
         (109, 138), (138, 174), (174, 219))

MEASURED_STANDIN = 3.0e-8             # largest |stand-in - float64| over CASE_NAMES: 2.97e-8 (ESTOI of k16_9218), rounded up
GPU_BOUND = 8 * MEASURED_STANDIN
MIN_MARGIN_DB = 0.01
KEEP_TRIP = 1024                      # frames that keep_frames' one workgroup of 1024 threads takes per loop trip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------- stage 1: the resampler
def taps():
    """5 * firwin(161, 1/8, window=('kaiser', 5.0)) with numpy alone: windowed sinc, DC gain 1, times 5."""
    m = np.arange(161, dtype=np.float64) - 80.0
    h = 0.125 * np.sinc(0.125 * m) * np.kaiser(161, 5.0)
    return 5.0 * (h / h.sum())


def resample(x, f32=False):
    """16 kHz -> 10 kHz: out[n] = sum_t h[t] xup[8 n + 80 - t], xup[5 m] = x[m], zero outside; ceil(5 L / 8) samples."""
    x = np.asarray(x, dtype=np.float64)
    L = x.size
    n_out = -(-5 * L // 8)
    h = taps()
    out = np.zeros(n_out, dtype=np.float64)
    c = 8 * np.arange(n_out, dtype=np.int64) + 80
    for t in range(161):                                  # ascending taps: the kernel's order
        num = c - t
        ok = (num % 5 == 0) & (num >= 0) & (num < 5 * L)
        out[ok] += h[t] * x[num[ok] // 5]
    return out.astype(np.float32).astype(np.float64) if f32 else out


# ---------------------------------------------------------------------------------------------- stage 2: silent frames
def window(periodic=False):
    if periodic:
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FRAME) / N_FRAME)
    return np.hanning(N_FRAME + 2)[1:-1]


def frame_starts(n, take_last=False):
    """0, 128, ... with i < n - 256 (strict); ``take_last`` (a mutant): i <= n - 256."""
    return np.arange(0, n - N_FRAME + (1 if take_last else 0), HOP, dtype=np.int64) if n >= N_FRAME else np.zeros(0, np.int64)


def frames_of(x, w, take_last=False):
    starts = frame_starts(x.size, take_last)
    if starts.size == 0:
        return np.zeros((0, N_FRAME))
    return w[None, :] * x[starts[:, None] + np.arange(N_FRAME)[None, :]]


def energies(x, periodic=False, take_last=False):
    """e_i = 20 log10(|w x_i| + eps) of every frame of x (10 kHz domain)."""
    f = frames_of(np.asarray(x, dtype=np.float64), window(periodic), take_last)
    return 20.0 * np.log10(np.linalg.norm(f, axis=1) + EPS)


def keep_mask(x, dyn=DYN_RANGE, trip=None, **kw):
    """``trip`` (the mutants of LONG_MUTANTS): a kept-frame pass that goes wrong behind its first KEEP_TRIP frames"""
    e = energies(x, **kw)
    if e.size == 0:
        return np.zeros(0, dtype=bool)
    top = np.max(e[:KEEP_TRIP]) if trip == "max_of_first_trip" else np.max(e)
    mask = (top - dyn - e) < 0
    if trip == "frames_of_one_trip":
        mask[KEEP_TRIP:] = False
    if trip == "scan_not_carried":                          # the last trip's frames from position 0, the count its own
        mask[:(e.size - 1) // KEEP_TRIP * KEEP_TRIP] = False
    return mask


def margin_10k(x):
    """smallest |e_i - (max e - 40)| in dB; inf without frames"""
    e = energies(x)
    return float(np.min(np.abs(e - (np.max(e) - DYN_RANGE)))) if e.size else float("inf")


def margin(x, fs):
    """the margin of a clean input at its own rate"""
    x = np.asarray(x, dtype=np.float64)
    return margin_10k(resample(x) if fs == 16000 else x)


def overlap_add(fr):
    """kept windowed frames (n, 256) -> (n - 1) 128 + 256 samples"""
    n = fr.shape[0]
    if n == 0:
        return np.zeros(0)
    out = np.zeros((n - 1) * HOP + N_FRAME)
    for q in range(n):
        out[q * HOP:q * HOP + N_FRAME] += fr[q]
    return out


def remove_silent(x, y, dyn=DYN_RANGE, periodic=False, take_last=False, decide_from_y=False, f32=False, trip=None):
    """-> x_sil, y_sil, frames, kept"""
    w = window(periodic)
    mask = keep_mask(y if decide_from_y else x, dyn, trip, periodic=periodic, take_last=take_last)
    xs = overlap_add(frames_of(x, w, take_last)[mask])
    ys = overlap_add(frames_of(y, w, take_last)[mask])
    if f32:
        xs, ys = (v.astype(np.float32).astype(np.float64) for v in (xs, ys))
    return xs, ys, int(mask.size), int(mask.sum())


# ---------------------------------------------------------------------------------------------- stage 3: band spectra
def band_edges():
    """(lo, hi) bins of the 15 third-octave bands on the grid k * 10000 / 512, upper bin excluded"""
    f = np.arange(NFFT // 2 + 1) * (FS / NFFT)
    out = []
    for j in range(NUM_BANDS):
        lo = MIN_FREQ * 2.0 ** ((2 * j - 1) / 6.0)
        hi = MIN_FREQ * 2.0 ** ((2 * j + 1) / 6.0)
        out.append((int(np.argmin(np.abs(f - lo))), int(np.argmin(np.abs(f - hi)))))
    return tuple(out)


def _basis32():
    """the kernel's basis: (w[k] cos, -w[k] sin)(2 pi f k / 512) for bins 7 .. 218, phase reduced exactly, rounded once"""
    k = np.arange(N_FRAME, dtype=np.int64)[:, None]
    f = np.arange(F0, F1, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((f * k) % NFFT).astype(np.float64) / NFFT
    w = window()[:, None]
    return (w * np.cos(ang)).astype(np.float32), (-w * np.sin(ang)).astype(np.float32)


def _chain32(A, Bm):
    """A (m, 256) float32 times Bm (256, n) float32 as the matrix cores form it: one ordered float32 chain over k per value"""
    acc = np.zeros((A.shape[0], Bm.shape[1]), dtype=np.float32)
    for k in range(A.shape[1]):
        acc = acc + A[:, k:k + 1] * Bm[k:k + 1, :]
    return acc


def band_spectra(x_sil, edges=EDGES, periodic=False, take_last=False, f32=False):
    """(15, M) band magnitudes of the frames of x_sil"""
    starts = frame_starts(x_sil.size, take_last)
    if starts.size == 0:
        return np.zeros((len(edges), 0))
    raw = x_sil[starts[:, None] + np.arange(N_FRAME)[None, :]]
    if f32:
        c, s = _basis32()
        a = raw.astype(np.float32)
        re, im = _chain32(a, c).astype(np.float64), _chain32(a, s).astype(np.float64)
        power = np.zeros((raw.shape[0], NFFT // 2 + 1))
        power[:, F0:F1] = re * re + im * im
    else:
        spec = np.fft.rfft(raw * window(periodic)[None, :], n=NFFT, axis=1)
        power = spec.real ** 2 + spec.imag ** 2
    return np.stack([np.sqrt(power[:, lo:hi].sum(axis=1)) for lo, hi in edges])


# ---------------------------------------------------------------------------------------------- stage 4: segments
def segment_blocks(X, n_seg=N_SEG):
    """(S, 15, n_seg): frames m - n_seg .. m - 1 for m = n_seg .. M"""
    M = X.shape[1]
    return np.stack([X[:, m - n_seg:m] for m in range(n_seg, M + 1)])


def _unit(v, axis):
    v = v - v.mean(axis=axis, keepdims=True)
    return v / (np.linalg.norm(v, axis=axis, keepdims=True) + EPS)


def stoi_from_bands(X, Y, n_seg=N_SEG, clip=True):
    xs, ys = segment_blocks(X, n_seg), segment_blocks(Y, n_seg)
    alpha = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + EPS)
    yp = alpha * ys
    if clip:
        yp = np.minimum(yp, xs * (1.0 + 10.0 ** (BETA_DB / 20.0)))
    return float(np.sum(_unit(xs, 2) * _unit(yp, 2)) / (xs.shape[0] * xs.shape[1]))


def estoi_from_bands(X, Y, n_seg=N_SEG, columns_first=False):
    xs, ys = segment_blocks(X, n_seg), segment_blocks(Y, n_seg)
    order = (1, 2) if columns_first else (2, 1)
    for axis in order:
        xs, ys = _unit(xs, axis), _unit(ys, axis)
    return float(np.sum(xs * ys / n_seg) / xs.shape[0])


# ---------------------------------------------------------------------------------------------- the whole score
MUTANTS = {
    "dyn_range_30": dict(dyn=30.0),
    "last_frame_taken": dict(take_last=True),
    "periodic_window": dict(periodic=True),
    "band_edge_off_by_one": dict(edges=EDGES[:5] + ((22, 28), (28, 34)) + EDGES[7:]),
    "no_clipping": dict(clip=False),
    "segments_of_29": dict(n_seg=29),
    "columns_before_rows": dict(columns_first=True),
    "decision_from_y": dict(decide_from_y=True),
}
# what a kept-frame pass does when it goes wrong past one trip of KEEP_TRIP frames; only a row of more frames can tell
LONG_MUTANTS = {
    "max_of_first_trip": dict(trip="max_of_first_trip"),      # the keep threshold from the maximum over frames 0 .. 1023
    "frames_of_one_trip": dict(trip="frames_of_one_trip"),    # frames >= 1024 are never kept
    "scan_not_carried": dict(trip="scan_not_carried"),        # the second trip's list starts at position 0 again
}


def score(x, y, fs, f32=False, dyn=DYN_RANGE, take_last=False, periodic=False, edges=EDGES, clip=True, n_seg=N_SEG,
          columns_first=False, decide_from_y=False, trip=None):
    """-> dict(stoi, estoi, frames, kept, segments) of the processed y against the clean x (float32 samples at ``fs``)"""
    if fs not in (16000, 10000):
        raise ValueError("fs must be 16000 or 10000")
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError("x and y must be 1-D and of one length")
    if fs == 16000:
        x, y = resample(x, f32), resample(y, f32)
    xs, ys, n_frames, kept = remove_silent(x, y, dyn, periodic, take_last, decide_from_y, f32, trip)
    X = band_spectra(xs, edges, periodic, take_last, f32)
    Y = band_spectra(ys, edges, periodic, take_last, f32)
    M = X.shape[1]
    if M < n_seg:
        return dict(stoi=DEGENERATE, estoi=DEGENERATE, frames=n_frames, kept=kept, segments=0, M=M)
    return dict(stoi=stoi_from_bands(X, Y, n_seg, clip), estoi=estoi_from_bands(X, Y, n_seg, columns_first), frames=n_frames,
                kept=kept, segments=M - n_seg + 1, M=M)


# ---------------------------------------------------------------------------------------------- the shared inputs
def speech_pair(seed, n, fs, snr_db, off=0.5):
    """burst-gated harmonic "speech" x and y = x + white noise at snr_db, float32 (n,).  ``off``: the fraction of the 40 - 120 ms
    blocks that are gated 70 dB down (0: no gating, every frame is kept)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(fs)
    f0 = rng.uniform(100.0, 180.0) * (1.0 + 0.05 * np.sin(2 * np.pi * 3.0 * t + rng.uniform(0, 6.28)))
    ph = 2 * np.pi * np.cumsum(f0) / fs
    x = np.zeros(n)
    for h in range(1, 25):                                # every harmonic with a slow envelope of its own: the bands move apart
        env = 1.0 + 0.9 * np.sin(2 * np.pi * rng.uniform(2.0, 9.0) * t + rng.uniform(0, 6.28))
        x += rng.uniform(0.3, 1.0) / h ** 0.7 * env * np.sin(h * ph + rng.uniform(0, 6.28))
    # breath noise 20 dB down, so that no band of the clean signal holds window leakage alone (there the float32 product's
    # rounding is large against the band's own value, which is an ill-conditioned input, not a property of the kernels)
    x += np.sqrt(np.mean(x ** 2)) * 0.1 * rng.standard_normal(n)
    gate = np.ones(n)
    i, on = 0, True
    while i < n and off > 0:                              # alternating runs; the gated ones make up `off` of the time
        ln = int(rng.uniform(0.12, 0.28) * (1.0 - off if on else off) * fs) + 1
        if not on:
            gate[i:i + ln] = 10.0 ** (-70.0 / 20.0)
        i, on = i + ln, not on
    x = 0.1 * x / np.sqrt(np.mean(x ** 2)) * gate
    noise = rng.standard_normal(n)
    noise *= np.sqrt(np.mean(x ** 2) / np.mean(noise ** 2)) * 10.0 ** (-snr_db / 20.0)
    return x.astype(np.float32), (x + noise).astype(np.float32)


def loud_tail_pair(seed, n, fs, snr_db, off, blocks):
    """``speech_pair`` at 10 kHz under a piecewise gain, the same for x and y: the last fifth times 2, so the loudest frame
    lies there, and 60 ms blocks near the sample offsets ``blocks`` (each moved on to the first place whose frames all lie
    within 10 dB of the first part's loudest) brought to the level halfway between the keep threshold and the threshold
    that the maximum over frames 0 .. KEEP_TRIP - 1 alone would give.  The true rule drops the blocks; the wrong one keeps
    them."""
    assert fs == FS
    x, y = (v.astype(np.float64) for v in speech_pair(seed, n, fs, snr_db, off))
    gain = np.ones(n)
    gain[n - n // 5:] = 2.0
    e = energies(x * gain)
    first, top = np.max(e[:KEEP_TRIP]), np.max(e)
    level = top - DYN_RANGE - 0.5 * (top - first)
    for s0 in blocks:
        f0 = s0 // HOP
        while np.min(e[f0 - 2:f0 + 7]) < first - 10.0:
            f0 += 1
        assert f0 + 7 < KEEP_TRIP
        # frames f0, f0 + 1, f0 + 2 lie inside samples 128 f0 .. 128 f0 + 599
        gain[f0 * HOP:f0 * HOP + 600] *= 10.0 ** ((level - np.mean(e[f0:f0 + 3])) / 20.0)
    return (x * gain).astype(np.float32), (y * gain).astype(np.float32)


def committed_pair():
    """the committed 48100-sample utterance: clean, and babble at -5 dB; 16 kHz"""
    load = lambda name: np.load(os.path.join(GOLDEN, name))["samples"].astype(np.float32) / 32768.0   # noqa: E731
    return load("utt_sa1_clean.npz"), load("utt_sa1.npz")


# name -> (fs, samples, snr, gated fraction, seed): the smallest shapes that can still go wrong.  4097 ungated samples at
# 10 kHz are 31 frames, all kept: exactly one segment; 4096 are 30 frames: no segment.  The 16 kHz lengths cover L mod 8 =
# 0 .. 7.  A row of 38 .. 57 frames cannot lose a third of them and keep 31, so the short rows are gated lightly (or
# heavily, to fall below 30 frames through the removal), and the rows long enough lose between a third and two thirds.
_SPECS = {
    "k10_4097_one_segment": (10000, 4097, 20.0, 0.0, 11),
    "k10_4096_no_segment": (10000, 4096, 5.0, 0.0, 12),
    "k10_6000_light": (10000, 6003, 5.0, 0.12, 13),
    "k10_6000_heavy": (10000, 5999, -5.0, 0.5, 14),
    "k10_9001_half": (10000, 9001, 5.0, 0.45, 15),
    "k16_8192": (16000, 8192, 20.0, 0.1, 20),
    "k16_8705": (16000, 8705, 5.0, 0.1, 21),
    "k16_9218": (16000, 9218, -5.0, 0.1, 22),
    "k16_9731": (16000, 9731, 20.0, 0.5, 23),
    "k16_10244": (16000, 10244, 5.0, 0.12, 24),
    "k16_10757": (16000, 10757, -5.0, 0.12, 25),
    "k16_11270": (16000, 11270, 20.0, 0.15, 26),
    "k16_11999": (16000, 11999, 5.0, 0.15, 27),
    "k16_16000_half": (16000, 16000, -5.0, 0.45, 28),
}
CASE_NAMES = tuple(_SPECS) + ("committed",)

# The cases past one trip, in a table of their own (MEASURED_STANDIN is measured over CASE_NAMES): more than 256 frames
# (invert_kept's second workgroup), more than KEEP_TRIP frames (keep_frames' second trip; an evaluation utterance of 14 s or
# more), with frames dropped on both sides of frame 1024, at both rates, and one at -5 dB.
_LONG_SPECS = {
    "k10_60000_mid": (10000, 60000, 20.0, 0.3, 73),
    "k10_141100": (10000, 141100, 20.0, 0.15, 62),
    "k10_211650_both_sides": (10000, 211650, 20.0, 0.45, 61),
    "k16_230003": (16000, 230003, 20.0, 0.15, 63),
    "k16_345004_both_sides": (16000, 345004, 20.0, 0.30, 63),
    "k10_166700_noisy": (10000, 166700, -5.0, 0.10, 52),
}
# name -> speech_pair's arguments and the sample offsets of loud_tail_pair's blocks
_LOUD_TAIL = {"k10_170000_loud_tail": (10000, 170000, 20.0, 0.15, 61, (20000, 55000, 90000, 120000))}
LOUD_TAIL_CASE = "k10_170000_loud_tail"
LONG_CASE_NAMES = tuple(_LONG_SPECS) + tuple(_LOUD_TAIL)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (fs, x, y) float32, read-only"""
    if name == "committed":
        fs, (x, y) = 16000, committed_pair()
    elif name in _LOUD_TAIL:
        fs, n, snr, off, seed, blocks = _LOUD_TAIL[name]
        x, y = loud_tail_pair(seed, n, fs, snr, off, blocks)
    else:
        fs, n, snr, off, seed = _SPECS[name] if name in _SPECS else _LONG_SPECS[name]
        x, y = speech_pair(seed, n, fs, snr, off)
    x.setflags(write=False), y.setflags(write=False)
    return fs, x, y


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 score of a case, computed once"""
    fs, x, y = case(name)
    return score(x, y, fs)


@functools.lru_cache(maxsize=None)
def case_margin(name):
    fs, x, _ = case(name)
    return margin(x, fs)


# ---------------------------------------------------------------------------------------------- the checks of a result
# What the GPU tests assert of ``d`` (STOI, ESTOI as floats) and ``info`` (frames, kept, segments as ints) of a case; the CPU
# tests hand the same functions a mutant's result to show that they can fail.
def check_info(name, info):
    ref = reference(name)
    assert case_margin(name) >= MIN_MARGIN_DB
    assert [int(v) for v in info] == [ref["frames"], ref["kept"], ref["segments"]]


def score_error(name, d):
    ref = reference(name)
    return max(abs(float(d[0]) - ref["stoi"]), abs(float(d[1]) - ref["estoi"]))


def check_d(name, d):
    assert score_error(name, d) <= GPU_BOUND


def check_scores(name, d, info, label=""):
    """-> |d - float64|, after printing it"""
    err = score_error(name, d)
    print("%s%-22s info %s  stoi %.9f estoi %.9f  |d - float64| = %.3g (bound %.3g)"
          % (label, name, [int(v) for v in info], float(d[0]), float(d[1]), err, GPU_BOUND))
    check_info(name, info)
    check_d(name, d)
    return err
