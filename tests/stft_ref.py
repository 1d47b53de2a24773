"""The oracle of the whole-utterance STFT tests (csrc/stft.hip: ``frames::framed_dft`` -- the ``FrameRows`` gather, ``dft_basis``,
``igemm::launch<128, 128>`` -- and the four epilogues behind ``ops.stft`` / ``ops.stft_complex``): a float64 framed DFT, the
launch plan RESTATED from ``gemm_ref.gemm_plan``'s pieces, the case list, a float32 CPU twin with its mutants and one
assertion function per tier.  An assertion function takes the implementation under test as a callable
``impl(what, wave, cfg)`` (``what``: one of WHATS; ``wave``: float32 (B, L); ``cfg``: the case's n_fft, hop, pad, fs, eps and
statistics) that returns a numpy array: tests/test_stft_gpu.py passes the HIP path, tests/test_stft_cpu.py passes the twin
(every bound must be within reach of correct float32 arithmetic) and its mutants (every assertion must be able to fail).

Reference.  The float32 wave is framed explicitly, frame t of row b = wave[b][t hop : t hop + n_fft] with zeros from sample L
on (the reference's end pad of one hop, by its own float test, ``end_pad``).  The basis is built in float64 the way
csrc/frames.h defines it: periodic Hann 0.5 - 0.5 cos(2 pi k / N) and the exactly reduced phase r = (f k) % N,
basis[k][2f] = hann cos(2 pi r / N), basis[k][2f + 1] = -hann sin(2 pi r / N), with the exact zeros forced where 4r % N == 0
(cos) and 2r % N == 0 (sin).  This float64 basis rounds to the same float32 values as an 80-bit evaluation for N = 32, 96,
512 and 1024; an unreduced cos(2 pi f k / N) does not.  The spectrum is the float64 product frames @ basis.  Nothing is taken
from ``oracle/frontend.py::stft`` (the float32 restatement of the original), which serves the frame COUNT only.

Three tiers, one assertion function each.

* IMPULSE (``check_impulse``; every configuration and mode).  Waves that are zero except for impulses +-2^j, at least n_fft
  apart within a row: every frame holds at most one, X[b][t][f] = a basis[p - t hop][f], and no summation order or schedule
  rounds anything.  Bound: |got - ref| <= 2^-23 |ref| element-wise -- one float32 ulp, for the device's cospi / sinpi against
  numpy's -- and EXACT zero wherever the reference is zero (frames that see no impulse, the sin columns of DC and Nyquist, the
  window's zero at k = 0).  Power: a^2 (c^2 + s^2) is exact up to the basis' ulp (2 2^-23 on the squares) and 3 roundings
  (3 2^-24): 4 2^-23 P.  Log: that dP through the feature bound below; where P = 0, float32(log(float64(float32(eps)))) within
  2 ulp.  Impulses sit where indexing goes wrong: sample 0 and L - 1 of every row (sample 0 of row b + 1 is what a last frame
  of row b that runs into the end pad would read), the first and last sample of every frame that starts on a 128-row tile
  boundary of M = B T, k = 0 and k = n_fft - 1 of every row's last frame; as many waves are made as it takes to place them all.
* ROUNDING (``check_rounding``).  White noise, and a signal with a 60 dB spectral tilt (linear in dB from DC to Nyquist),
  peak-normalised with numpy.  Element-wise |got - ref| <= (n_fft + 41) 2^-24 S, S = |frames| |basis| in float64: gemm_ref's
  bound (gamma_K of one ordered chain, 32 more additions for the pieces of a split tile, head-room of 8) plus one for the
  basis' own rounding -- derived, not measured; where S = 0 the result is 0.  Aggregate, because the element bound alone
  passes a basis evaluated in float32: the relative Frobenius error of the spectrum must not exceed 4 x that of the float32
  twin run as ONE sequential chain per element on the same inputs (the least accurate correct float32 order; the factor
  covers another order and the pieces of split tiles).  The workspace's own spectrum is checked with it: its first 2F
  columns are the output bit for bit, its padding columns are zero.
* FEATURES (``check_features``).  The element bound E above, propagated:
  power dP <= 2 (|re| E_re + |im| E_im) + E_re^2 + E_im^2 + 2^-22 P;
  log |d log| <= dP / (P + eps - dP) + 2^-22 max(1, |log(P + eps)|) (the float32 add of eps, and logf);
  standardised (d log + 2^-23 (|v| + |mean|)) / (std + norm_eps) + 2^-23 |out|.
  An element whose log bound exceeds 0.05 is UNCHECKED; the share of such elements is asserted on the reference alone: 0
  for the white-noise cases, at most 1 % for the tilted ones.  The same 4 x twin aggregate holds on the log features.
  Which cases can carry this tier follows from the bound itself, on the reference alone.  A bin is checked when |X| exceeds
  about 40 E, and E grows with (n_fft + 41) S.  A white spectrum's power is exponentially distributed (DC and Nyquist, being
  real, chi-square with ONE degree of freedom: each such element is unchecked with a probability of some 0.4 % at n_fft 256),
  so some share of a white spectrum is unchecked however it is drawn: 0.004 % of 50 796 elements at n_fft 32, 0.014 % at 256,
  0.23 % at n_fft 1024 (``round-1024x256-B3``).  The white feature cases are therefore SMALL (833 to 2397 elements, at n_fft
  32, 96 and 512) and their reference has none.  The 60 dB tilt leaves 0.79 % unchecked at n_fft 32, 2.4 % at 96 and 40 % at
  1024: the tilted feature case is at n_fft 32.  The other configurations have the impulse tier's power and log, and the
  silence case.
  Silence: an all-zero wave gives float32(log(float64(float32(eps)))) within 2 ulp in mode 0, exactly 0 in mode 1, the
  spectrum and the standardised features' numerator.

Measured.  MI355X | float32 twin in numpy's order | as one sequential chain.  Worst element error / bound, then the relative
Frobenius error of the spectrum, then (feature cases) of the log features:
  round-1024x256-B3    0.0015 | 0.0023 | 0.0063    2.11e-07 | 3.08e-07 | 5.73e-07
  round-1024x256-tilt  0.0027 | 0.0041 | 0.0086    2.14e-07 | 3.03e-07 | 5.61e-07
  round-1024x256-43h   0.0010 | 0.0019 | 0.0044    2.11e-07 | 3.07e-07 | 5.64e-07
  round-512x100-B3     0.0040 | 0.0071 | 0.0091    2.08e-07 | 2.87e-07 | 4.05e-07
  round-96x32-B3       0.0336 | 0.0398 | 0.0398    1.56e-07 | 1.71e-07 | 1.74e-07
  round-96x100-B3      0.0298 | 0.0298 | 0.0357    1.73e-07 | 1.73e-07 | 1.77e-07
  round-32x8-B3        0.0484 | 0.0484 | 0.0585    9.84e-08 | 9.84e-08 | 1.04e-07
  round-32x8-feat      0.0465 | 0.0465 | 0.0457    9.66e-08 | 9.40e-08 | 1.02e-07    5.68e-07 | 2.30e-07 | 5.16e-07
  round-32x8-tilt      0.0754 | 0.0754 | 0.0632    9.86e-08 | 9.86e-08 | 1.01e-07    1.44e-06 | 1.43e-06 | 2.21e-06
  round-32x8-full      0.0761 | 0.0761 | 0.0783    9.85e-08 | 9.85e-08 | 1.03e-07
  round-1024x1024-B3   0.0011 | 0.0017 | 0.0041    2.11e-07 | 3.06e-07 | 5.61e-07
  round-256x64-B3      0.0112 | 0.0192 | 0.0191    2.04e-07 | 2.83e-07 | 2.86e-07
  round-96x32-feat     0.0215 | 0.0215 | 0.0214    1.79e-07 | 1.78e-07 | 1.76e-07    3.20e-07 | 2.91e-07 | 2.96e-07
  round-512x100-feat   0.0031 | 0.0039 | 0.0044    2.07e-07 | 2.75e-07 | 3.89e-07    2.71e-07 | 2.74e-07 | 3.53e-07
  round-256x64-sched   0.0242 | 0.0242 | 0.0242    2.83e-07 | 2.83e-07 | 2.86e-07
  center-1024x256      0.0015 | 0.0020 | 0.0057    2.10e-07 | 3.05e-07 | 5.70e-07
  center-256x64        0.0094 | 0.0154 | 0.0154    2.06e-07 | 2.86e-07 | 2.88e-07
(the element bound is the worst case of n_fft aligned rounding errors; random ones add up to its square root.  Figures that
agree to four digits are elements with one dominant product.)  Features, worst error / bound on the MI355X: power 0.003 to 0.069,
log 0.003 to 0.092, standardised 0.004 to 0.155.  Impulse tier: of the 1 583 826 non-zero elements of all impulse cases, 0
differ from float32(reference) on the MI355X, and 0 for the twin (whose basis IS float32(reference)).  The mutants
(tests/test_stft_cpu.py): a basis with float32 cos / sin / Hann and an unreduced phase stays at 0.24 (n_fft 1024), 0.63 (96)
and 0.59 (32) of the element bound and is 63 x, 23 x and 12 x the chain twin in the aggregate; operands rounded to bf16 are
8.5 x the element bound at n_fft 1024 and 3900 x to 22 000 x the twin in the aggregate.
"""
import functools
import math
import zlib

import numpy as np

import gemm_ref as G
import head_ref as H

FAMILY = "stft"
CSRC = G.CSRC
U = 2.0 ** -24                            # unit round-off of float32
ULP = 2.0 ** -23
TWIN_FACTOR = 4.0
UNCHECKED_AT = 0.05
WHATS = ("complex", "legacy", "power", "log", "std", "workspace", "center", "lps")

# The lines of the source the plan restatement and the framing rest on, as (file, line, text): tests/test_stft_cpu.py::
# test_cited_lines_hold fails when an edit moves one.
CITES = [
    ("stft.hip", 27, "const int b = x / T, fr = x - b * T;"),
    ("stft.hip", 28, "const long idx = (long)fr * hop + k;"),
    ("stft.hip", 29, "if (idx < L) t = p[(long)b * L + idx];"),
    ("stft.hip", 41, "if (c < 2 * F) {"),
    ("stft.hip", 44, "v = (float)((c & 1) ? -win * ph.sin() : win * ph.cos());"),
    ("stft.hip", 104, "FrameRows a{wave, L, M, n_fft, T, hop};"),
    ("stft.hip", 105, "igemm::ColPlain<4> b{W, ld, ld, n_fft, 0};"),
    ("stft.hip", 107, "return igemm::launch<128, 128>(a, b, e, M, ld, n_fft, 1, s, ws + w.slab, /*allow_bf16=*/false);"),
    ("frames.h", 12, "static inline bool ok_n_fft(int n_fft) { return n_fft >= 32 && n_fft % 32 == 0; }"),
    ("frames.h", 15, "(long)(d->T - 1) * d->hop + d->n_fft <= d->L + d->hop;"),
    ("frames.h", 19, "return 0.5 - 0.5 * cospi(2.0 * (double)k / (double)N);"),
    ("frames.h", 27, "const long fk = ((long)f * k) % N;"),
    ("frames.h", 62, "static inline int spectrum_ld(int n_fft) { return (2 * (n_fft / 2 + 1) + 3) / 4 * 4; }"),
    ("frames.h", 75, "w.S = w.W + align_up((size_t)n_fft * w.ld, 64);"),
]


# ------------------------------------------------------------------------------------------ frame count, layout, plan
def end_pad(L, n_fft, hop, fs=16e3):
    """the reference's test for its one-hop end pad, in its floats and its order of divisions"""
    v = L / fs / (n_fft / fs) / (hop / n_fft)
    return math.ceil(v) != int(v)


def n_frames(L, n_fft, hop, pad=True, fs=16e3):
    if pad and end_pad(L, n_fft, hop, fs):
        L = L + hop
    return (L - n_fft) // hop + 1


def spectrum_ld(n_fft):                   # frames.h (line 62)
    return (2 * (n_fft // 2 + 1) + 3) // 4 * 4


def ws_spectrum_offset(n_fft):            # frames.h spec_ws (line 75): floats in front of S within the workspace
    return -(-(n_fft * spectrum_ld(n_fft)) // 64) * 64


def stft_plan(B, T, n_fft):
    """the plan of stft.hip framed_dft (line 107): launch<128, 128> with M = B T, N = ld, K = n_fft, FrameRows (line 104) for A,
    ColPlain<4> (line 105) for the basis, the engine's slab always given"""
    ld = spectrum_ld(n_fft)
    d = dict(M=B * T, N=ld, K=n_fft, lda=n_fft, ldb=ld, ldc=ld, transA=0, transB=0, accumulate=0, split_k=1, relu_a=0, relu_b=0)
    p = G.gemm_plan(d, tile=128)
    assert p["tile"] == 128 and p["b_form"] == "ColPlain4" and p["kernel"] == "db512"
    p["a_form"] = "FrameRows"
    p["schedule"] = "both" if p["full_rounds"] >= 1 and p["rem"] > 0 else ("pool" if p["rem"] > 0 else "full")
    return p


# ------------------------------------------------------------------------------------------ the float64 reference
@functools.lru_cache(maxsize=None)
def basis64(n_fft, hann="periodic", sign=-1.0):
    """(n_fft, 2F) float64"""
    N, F = n_fft, n_fft // 2 + 1
    k, f = np.arange(N)[:, None], np.arange(F)[None, :]
    r = (f * k) % N
    c, s = np.cos(2.0 * np.pi * r / N), np.sin(2.0 * np.pi * r / N)
    q = (4 * r) % N == 0
    c[q] = np.array([1.0, 0.0, -1.0, 0.0])[(4 * r[q]) // N]
    s[(2 * r) % N == 0] = 0.0
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / (N if hann == "periodic" else N - 1))
    w[0] = 0.0
    W = np.empty((N, 2 * F))
    W[:, 0::2] = w[:, None] * c
    W[:, 1::2] = sign * w[:, None] * s
    W.setflags(write=False)
    return W


def frames_of(wave, n_fft, hop, T, offset=0, next_row=False):
    """(B T, n_fft) gather of wave (B, L), in the wave's dtype: zeros from sample L of a row on (``next_row``: whatever the
    flat buffer holds there, zeros behind its end); ``offset``: every index shifted by that many samples"""
    B, L = wave.shape
    flat = np.concatenate([wave.reshape(-1), np.zeros(hop + n_fft + 1, dtype=wave.dtype)])
    idx = (np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :] + offset)[None] + np.zeros((B, 1, 1), dtype=np.int64)
    flat_idx = np.minimum(np.arange(B)[:, None, None] * L + idx, flat.size - 1)
    out = flat[flat_idx]
    if not next_row:
        out = np.where(idx < L, out, 0)
    return out.reshape(B * T, n_fft).astype(wave.dtype)


def spectrum64(wave, n_fft, hop, T):
    """(X, S): the float64 spectrum (B T, 2F), (re, im) adjacent, and |frames| |basis|"""
    A = frames_of(wave, n_fft, hop, T).astype(np.float64)
    W = basis64(n_fft)
    return A @ W, np.abs(A) @ np.abs(W)


# ------------------------------------------------------------------------------------------ the cases
CASES = {}
CONFIGS = ((1024, 256), (512, 100), (96, 32), (96, 100), (32, 8), (1024, 1024), (256, 64))


def _case(name, n_fft, hop, B, L, why, pad=True, signal="impulse", features=False, unchecked_max=None, reach=None):
    assert name not in CASES, name
    CASES[name] = dict(name=name, n_fft=n_fft, hop=hop, B=B, L=L, pad=pad, fs=16e3, eps=1e-8, norm_eps=1e-3, signal=signal,
                       features=features, unchecked_max=unchecked_max, why=why, reach=reach or {})
    return name


def case_T(c):
    return n_frames(c["L"], c["n_fft"], c["hop"], c["pad"], c["fs"])


IMPULSE = []
for _n, _h in CONFIGS:
    _t = "%dx%d" % (_n, _h)
    IMPULSE += [
        _case("imp-%s-T1" % _t, _n, _h, 1, _n, "L = n_fft: T = 1, M = 1", pad=False, reach=dict(M=1)),
        _case("imp-%s-T1-B3" % _t, _n, _h, 3, _n, "T = 1 with three rows: b = x / T is x itself", pad=False, reach=dict(M=3)),
        _case("imp-%s-j-exact" % _t, _n, _h, 3, _n + 7 * _h, "n_fft + 7 hop exactly, rows of different content"),
        _case("imp-%s-j-minus" % _t, _n, _h, 3, _n + 7 * _h - 1, "one sample short of it: the last frame runs into the end pad"),
        _case("imp-%s-j-plus" % _t, _n, _h, 3, _n + 7 * _h + 1, "one sample over"),
        _case("imp-%s-16000" % _t, _n, _h, 1, 16000, "one second"),
    ]
IMPULSE += [
    _case("imp-1024x256-43h", 1024, 256, 1, 43 * 256, "an exact hop multiple at which the reference's float test pads", reach=dict(T=41)),
    _case("imp-1024x256-44h", 1024, 256, 1, 44 * 256, "its neighbour, which does not", reach=dict(T=41)),
    _case("imp-1024x256-43h-nopad", 1024, 256, 1, 43 * 256, "pad_at_end = False", pad=False, reach=dict(T=40)),
    _case("imp-1024x256-44h-nopad", 1024, 256, 1, 44 * 256, "pad_at_end = False", pad=False, reach=dict(T=41)),
    _case("imp-1024x256-M60", 1024, 256, 1, 16000 - 1, "M = 60: inside one 128-row tile, all 9 tiles in the stream-K pool",
          reach=dict(M=60, schedule="pool", ntm=1, ntn=9)),
    _case("imp-1024x256-M128", 1024, 256, 2, 1024 + 63 * 256, "M = 128: row 1 ends with the tile", pad=False, reach=dict(M=128, ntm=1)),
    _case("imp-1024x256-M129", 1024, 256, 3, 1024 + 42 * 256 + 5, "M = 129: the last frame of the last row starts a tile of its own",
          pad=False, reach=dict(M=129, ntm=2)),
    _case("imp-1024x256-M273", 1024, 256, 3, 24000, "M crosses two tile edges, inside rows", reach=dict(M=273, ntm=3)),
    _case("imp-32x8-full", 32, 8, 3, 160024, "469 tiles of one column: data-parallel rounds only",
          reach=dict(schedule="full", ntn=1, ktiles=1)),
    _case("imp-256x64-sched", 256, 64, 22, 64000, "a full round of 512 tiles and a stream-K remainder of 4 split tiles",
          reach=dict(schedule="both", full_rounds=1, rem=4, split_tiles=4)),
]

ROUNDING = [
    _case("round-1024x256-B3", 1024, 256, 3, 16000, "the flagship configuration, 18 pool tiles", signal="white", reach=dict(schedule="pool")),
    _case("round-1024x256-tilt", 1024, 256, 1, 16000, "60 dB tilt: the spectrum's bound on low-power bins", signal="tilt"),
    _case("round-1024x256-43h", 1024, 256, 1, 43 * 256, "the padded exact multiple", signal="white"),
    _case("round-512x100-B3", 512, 100, 3, 16000, "hop does not divide n_fft", signal="white"),
    _case("round-96x32-B3", 96, 32, 3, 16000, "n_fft no power of two: the phase reduction is a real modulo; ld = 100", signal="white"),
    _case("round-96x100-B3", 96, 100, 3, 4001, "hop > n_fft: samples no frame reads", signal="white"),
    _case("round-32x8-B3", 32, 8, 3, 4001, "one K tile, N = 36 inside one tile", signal="white"),
    _case("round-32x8-feat", 32, 8, 3, 400, "white features, M = 141 across a tile edge", signal="white", features=True, unchecked_max=0.0),
    _case("round-32x8-tilt", 32, 8, 3, 4001, "60 dB tilt with every bin within reach of the bound", signal="tilt", features=True,
          unchecked_max=0.01),
    _case("round-32x8-full", 32, 8, 3, 160024, "data-parallel rounds only", signal="white", reach=dict(schedule="full")),
    _case("round-1024x1024-B3", 1024, 1024, 3, 16000, "hop = n_fft", signal="white"),
    _case("round-256x64-B3", 256, 64, 3, 16000, "8 K tiles, 18 pool tiles", signal="white"),
    _case("round-96x32-feat", 96, 32, 1, 600, "white features, the modulo phase", signal="white", features=True, unchecked_max=0.0),
    _case("round-512x100-feat", 512, 100, 1, 1000, "white features on 16 K tiles", signal="white", features=True, unchecked_max=0.0),
    _case("round-256x64-sched", 256, 64, 22, 64000, "full round + split stream-K tiles", signal="white",
          reach=dict(schedule="both", full_rounds=1, rem=4, split_tiles=4)),
]
SCHEDULE_CASE = "round-256x64-sched"
SILENCE = [_case("silence-1024x256", 1024, 256, 3, 16000, "all-zero wave", signal="zero"),
           _case("silence-96x32", 96, 32, 1, 500, "all-zero wave", signal="zero")]
CENTER = [_case("center-1024x256", 1024, 256, 1, 16000, "stft_pytorch(center=True)", signal="white"),
          _case("center-256x64", 256, 64, 1, 4001, "stft_pytorch(center=True)", signal="white")]


def cfg_of(c):
    """what an implementation is told about a case"""
    F = c["n_fft"] // 2 + 1
    rng = np.random.default_rng(zlib.crc32(("stat" + c["name"]).encode()))
    mean = (-3.0 + 2.0 * rng.standard_normal(F)).astype(np.float32)
    std = rng.uniform(0.5, 2.0, F).astype(np.float32)
    std[F // 3] = 0.0                                     # a bin that never varied: norm_eps alone divides
    return dict(n_fft=c["n_fft"], hop=c["hop"], pad=c["pad"], fs=c["fs"], eps=c["eps"], norm_eps=c["norm_eps"], mean=mean, std=std)


def plan_of(name):
    c = CASES[name]
    p = stft_plan(c["B"], case_T(c), c["n_fft"])
    p["M"], p["T"] = c["B"] * case_T(c), case_T(c)
    return p


# ------------------------------------------------------------------------------------------ the signals
def _peak(x):
    x = x.astype(np.float32)
    return (x / np.abs(x).max(axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=4)
def signal(name):
    c = CASES[name]
    B, L = c["B"], c["L"]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if c["signal"] == "zero":
        return np.zeros((B, L), dtype=np.float32)
    x = rng.standard_normal((B, L))
    if c["signal"] == "tilt":                             # 60 dB down at Nyquist, linear in dB
        X = np.fft.rfft(x, axis=1)
        X *= 10.0 ** (-3.0 * np.arange(X.shape[1]) / (X.shape[1] - 1))
        x = np.fft.irfft(X, n=L, axis=1)
    else:
        assert c["signal"] == "white"
    x = _peak(x)
    x.setflags(write=False)
    return x


def impulse_waves(name):
    """-> [(wave (B, L) float32, [(b, p, a)])]: as many waves as it takes to place every required impulse, each with the
    required ones it has room for and random ones in what room is left; at least n_fft between two impulses of a row"""
    c = CASES[name]
    B, L, N, hop, T = c["B"], c["L"], c["n_fft"], c["hop"], case_T(c)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    need = []
    for b in range(B):
        mine = [0, L - 1, (T - 1) * hop, (T - 1) * hop + N - 1]
        if b > 0 and (T - 1) * hop + N > L:               # the first sample of this row a pad that runs on into it would read
            mine.insert(1, 0 if (T - 1) * hop < L else (T - 1) * hop - L + 1)      # (+ 1: k = 0 meets the window's zero)
        for m in range(0, B * T, 128):
            if m // T == b:
                mine += [(m % T) * hop, (m % T) * hop + N - 1]
        need += [(b, p) for p in dict.fromkeys(mine) if 0 <= p < L]
    waves = []
    while need:
        wave, placed, left = np.zeros((B, L), dtype=np.float32), [], []
        extra = [(int(b), int(p)) for b, p in zip(rng.integers(0, B, 4 * B + 8), rng.integers(0, L, 4 * B + 8))]
        for i, (b, p) in enumerate(need + extra):
            if all(q[0] != b or abs(q[1] - p) >= N for q in placed):
                a = float(rng.choice([-1.0, 1.0]) * 2.0 ** int(rng.integers(-6, 4)))
                wave[b, p] = a
                placed.append((b, p, a))
            elif i < len(need):
                left.append((b, p))
        assert len(left) < len(need)
        need = left
        waves.append((wave, placed))
    return waves


def impulse_reference(c, placed):
    """(B, T, F, 2) float64, exact: a basis[p - t hop] in every frame t that holds the impulse at p"""
    N, hop, T = c["n_fft"], c["hop"], case_T(c)
    W = basis64(N)
    ref = np.zeros((c["B"], T, N // 2 + 1, 2))
    for b, p, a in placed:
        for t in range(max(0, -(-(p - N + 1) // hop)), min(T - 1, p // hop) + 1):
            ref[b, t, :, 0] += a * W[p - t * hop, 0::2]
            ref[b, t, :, 1] += a * W[p - t * hop, 1::2]
    return ref


# ------------------------------------------------------------------------------------------ the assertion functions
def _log(tag, msg):
    if tag is not None:
        H.log_line("stft %-12s %s" % (tag, msg))


def _eps32(c):
    return float(np.float32(c["eps"]))


def silence_log(c):
    return np.float32(np.log(np.float64(np.float32(c["eps"]))))


def _ulps(got, want):
    """distance in float32 ulps of ``want`` (a float32 scalar)"""
    return np.abs(got.astype(np.float64) - float(want)) / float(np.spacing(np.abs(np.float32(want))))


def log_bound(P, dP, eps):
    """|d log| of the feature tier: dP / (P + eps - dP) + 2^-22 max(1, |log(P + eps)|); inf where dP swallows the element"""
    den = P + eps - dP
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(den > 0, dP / np.where(den > 0, den, 1.0), np.inf)
    return rel + 2.0 ** -22 * np.maximum(1.0, np.abs(np.log(P + eps)))


def _within(name, what, got, ref, bound, mask=None):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, "%s %s: shape %s, expected %s" % (name, what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s %s: %d non-finite values" % (name, what, int((~np.isfinite(got)).sum()))
    err = np.abs(got - ref)
    bad = err > bound
    if mask is not None:
        bad &= mask
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s %s: %d of %d elements miss their bound; the first at %s: got %r, reference %r, bound %.3e" % (
            name, what, int(bad.sum()), bad.size, i, got[i], ref[i], np.broadcast_to(bound, ref.shape)[i]))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
    if mask is not None:
        ratio = np.where(mask, ratio, 0.0)
    return float(ratio.max()) if ratio.size else 0.0


def _views_agree(name, impl, wave, cfg, spec):
    """mode 2 and stft_complex of one utterance are views of one spectrum, bit for bit"""
    legacy = impl("legacy", wave, cfg)
    assert legacy.shape == (spec.shape[2], spec.shape[1], 2), "%s legacy: shape %s" % (name, legacy.shape)
    assert np.array_equal(legacy.view(np.uint32), np.ascontiguousarray(spec[0].transpose(1, 0, 2)).view(np.uint32)), \
        "%s: mode 2 is not the (F, T, 2) view of stft_complex's spectrum" % name


def check_impulse(impl, name, tag="gpu"):
    """-> (elements one ulp off float32(reference), non-zero elements)"""
    c, cfg = CASES[name], cfg_of(CASES[name])
    eps = _eps32(c)
    off = total = 0
    for wave, placed in impulse_waves(name):
        ref = impulse_reference(c, placed)
        spec = impl("complex", wave, cfg)
        assert spec.dtype == np.float32
        zero = ref == 0
        assert not (spec[zero] != 0).any(), "%s: %d elements are not zero where the spectrum is exactly zero, the first at %s" % (
            name, int((spec[zero] != 0).sum()), tuple(np.argwhere(zero & (spec != 0))[0]))
        _within(name, "spectrum", spec, ref, ULP * np.abs(ref))
        off += int((spec != ref.astype(np.float32)).sum())
        total += int((~zero).sum())
        if c["B"] == 1:
            _views_agree(name, impl, wave, cfg, spec)
        P = ref[..., 0] ** 2 + ref[..., 1] ** 2
        dP = 4.0 * ULP * P
        pw = impl("power", wave, cfg)
        assert not (pw[P == 0] != 0).any(), "%s: power is not zero where the spectrum is" % name
        _within(name, "power", pw, P, dP)
        lg = impl("log", wave, cfg)
        _within(name, "log-power", lg, np.log(P + eps), log_bound(P, dP, eps), mask=P > 0)
        if (P == 0).any():
            assert _ulps(lg[P == 0], silence_log(c)).max() <= 2, "%s: log(0 + eps) is %r, expected %r" % (
                name, lg[P == 0][0], silence_log(c))
    _log(tag, "%-26s impulse: %d of %d non-zero elements one ulp off float32(reference)" % (name, off, total))
    return off, total


def rel_fro(got, ref):
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - ref) / np.linalg.norm(ref))


@functools.lru_cache(maxsize=2)
def _round_reference(name):
    c = CASES[name]
    wave = signal(name)
    T = case_T(c)
    X, S = spectrum64(wave, c["n_fft"], c["hop"], T)
    E = (c["n_fft"] + 41) * U * S
    chain = twin_spectrum(wave, c["n_fft"], c["hop"], T, order="chain")
    return X, E, chain


def _feature_reference(c, cfg, X, E):
    eps = _eps32(c)
    re, im, Ere, Eim = X[:, 0::2], X[:, 1::2], E[:, 0::2], E[:, 1::2]
    P = re ** 2 + im ** 2
    dP = 2.0 * (np.abs(re) * Ere + np.abs(im) * Eim) + Ere ** 2 + Eim ** 2 + 2.0 ** -22 * P
    v = np.log(P + eps)
    dlog = log_bound(P, dP, eps)
    mean, std = cfg["mean"].astype(np.float64), cfg["std"].astype(np.float64)
    den = std + float(np.float32(cfg["norm_eps"]))
    out = (v - mean) / den
    dstd = (dlog + ULP * (np.abs(v) + np.abs(mean))) / den + ULP * np.abs(out)
    return dict(P=P, dP=dP, log=v, dlog=dlog, std=out, dstd=dstd, checked=dlog <= UNCHECKED_AT)


def unchecked_share(name):
    """the share of log-feature elements whose bound exceeds UNCHECKED_AT: a property of the reference alone"""
    c = CASES[name]
    X, E, _ = _round_reference(name)
    return float(1.0 - _feature_reference(c, cfg_of(c), X, E)["checked"].mean())


def element_ratio(got, X, E):
    """max of |got - ref| / bound over the elements whose bound is not zero"""
    return float((np.abs(np.asarray(got, dtype=np.float64) - X)[E > 0] / E[E > 0]).max())


def check_rounding(impl, name, tag="gpu"):
    """the spectrum of a noise case: element bound, exact zeros where S is 0, the 4 x twin aggregate, the workspace's padding
    columns -> dict of figures"""
    c, cfg = CASES[name], cfg_of(CASES[name])
    wave = signal(name)
    B, T, F = c["B"], case_T(c), c["n_fft"] // 2 + 1
    X, E, chain = _round_reference(name)
    spec = impl("complex", wave, cfg)
    assert spec.shape == (B, T, F, 2) and spec.dtype == np.float32, (name, spec.shape, spec.dtype)
    got = spec.reshape(B * T, 2 * F)
    assert not (got[E == 0] != 0).any(), "%s: non-zero where |frames| |basis| is zero" % name
    worst = _within(name, "spectrum", got, X, E)
    fig = dict(worst=worst, fro=rel_fro(got, X), fro_twin=rel_fro(chain, X))
    _log(tag, "%-26s spectrum: worst error / bound %.4f, relative Frobenius error %.3e (sequential float32 twin %.3e)" % (
        name, worst, fig["fro"], fig["fro_twin"]))
    assert fig["fro"] <= TWIN_FACTOR * fig["fro_twin"], "%s: relative Frobenius error %.3e, more than %g x the %.3e of a sequential " \
        "float32 chain" % (name, fig["fro"], TWIN_FACTOR, fig["fro_twin"])
    Sws = impl("workspace", wave, cfg)
    ld = spectrum_ld(c["n_fft"])
    assert Sws.shape == (B * T, ld), (name, Sws.shape)
    assert np.array_equal(Sws[:, :2 * F].view(np.uint32), got.view(np.uint32)), "%s: stft_complex is not the workspace's spectrum" % name
    assert not (Sws[:, 2 * F:] != 0).any(), "%s: the padding columns %d .. %d of the workspace spectrum are not zero" % (name, 2 * F, ld - 1)
    if B == 1:
        _views_agree(name, impl, wave, cfg, spec)
    return fig


def check_features(impl, name, tag="gpu"):
    """power, log-power and standardised log-power of a feature case -> dict of figures"""
    c, cfg = CASES[name], cfg_of(CASES[name])
    assert c["features"]
    wave = signal(name)
    B, T, F = c["B"], case_T(c), c["n_fft"] // 2 + 1
    X, E, chain = _round_reference(name)
    r = _feature_reference(c, cfg, X, E)
    share = float(1.0 - r["checked"].mean())
    assert share <= c["unchecked_max"], "%s: %.3f %% of the reference's elements have a log bound above %g" % (name, 100 * share, UNCHECKED_AT)
    shape = (B, T, F)
    fig = dict(unchecked=share)
    fig["power"] = _within(name, "power", impl("power", wave, cfg).reshape(B * T, F), r["P"], r["dP"])
    lg = impl("log", wave, cfg)
    assert lg.shape == shape, (name, lg.shape)
    lg = lg.reshape(B * T, F)
    fig["log"] = _within(name, "log-power", lg, r["log"], r["dlog"], mask=r["checked"])
    fig["std"] = _within(name, "standardised", impl("std", wave, cfg).reshape(B * T, F), r["std"], r["dstd"], mask=r["checked"])
    fig["fro_log"], fig["fro_log_twin"] = rel_fro(lg, r["log"]), rel_fro(twin_features(chain, "log", cfg), r["log"])
    _log(tag, "%-26s features: worst error / bound power %.4f log %.4f standardised %.4f; log features' relative Frobenius error "
         "%.3e (twin %.3e); unchecked %.4f %%" % (name, fig["power"], fig["log"], fig["std"], fig["fro_log"], fig["fro_log_twin"],
                                                 100 * share))
    assert fig["fro_log"] <= TWIN_FACTOR * fig["fro_log_twin"], "%s: log features' relative Frobenius error %.3e, more than %g x the " \
        "twin's %.3e" % (name, fig["fro_log"], TWIN_FACTOR, fig["fro_log_twin"])
    lps = impl("lps", wave, cfg)
    assert np.array_equal(lps.view(np.uint32), lg.reshape(shape).view(np.uint32)), "%s: log_power_spectrogram is not mode 0" % name
    return fig


def check_silence(impl, name):
    c, cfg = CASES[name], cfg_of(CASES[name])
    wave = signal(name)
    assert not wave.any()
    for what in ("complex", "power", "workspace"):
        out = impl(what, wave, cfg)
        assert out.size > 0 and not (out != 0).any(), "%s: %s of silence is not zero" % (name, what)
    lg = impl("log", wave, cfg)
    assert _ulps(lg, silence_log(c)).max() <= 2, "%s: log-power of silence is %r, expected %r" % (name, lg.flat[0], silence_log(c))
    sd = impl("std", wave, cfg).astype(np.float64)
    den = cfg["std"].astype(np.float64) + float(np.float32(cfg["norm_eps"]))
    ref = (float(silence_log(c)) - cfg["mean"].astype(np.float64)) / den
    _within(name, "standardised silence", sd, np.broadcast_to(ref, sd.shape),
            (2 * ULP * abs(float(silence_log(c))) + ULP * np.abs(cfg["mean"])) / den + ULP * np.abs(ref))


def check_center(impl, name, tag="gpu"):
    """stft_pytorch(center=True): the rounding tier against the float64 reference of the reflect-padded wave"""
    c, cfg = CASES[name], cfg_of(CASES[name])
    N, hop = c["n_fft"], c["hop"]
    assert c["B"] == 1 and (N / c["fs"]) * c["fs"] == N and int((hop / N) * N) == hop
    wave = signal(name)
    x = wave[0]
    if c["pad"] and end_pad(c["L"], N, hop, c["fs"]):
        x = np.concatenate([x, np.zeros(hop, dtype=np.float32)])
    x = np.pad(x, N // 2, mode="reflect")[None]
    T = n_frames(x.shape[1], N, hop, pad=False)
    X, S = spectrum64(x, N, hop, T)
    E = (N + 41) * U * S
    got = impl("center", wave, cfg)
    assert got.shape == (N // 2 + 1, T, 2), (name, got.shape)
    got = got.transpose(1, 0, 2).reshape(T, -1)
    worst = _within(name, "centred spectrum", got, X, E)
    fro, fro_twin = rel_fro(got, X), rel_fro(twin_spectrum(x, N, hop, T, order="chain"), X)
    _log(tag, "%-26s centred: worst error / bound %.4f, relative Frobenius error %.3e (twin %.3e)" % (name, worst, fro, fro_twin))
    assert fro <= TWIN_FACTOR * fro_twin, (name, fro, fro_twin)
    return worst


# ------------------------------------------------------------------------------------------ the float32 CPU twin
MUTANTS = ("frame_offset", "pad_next_row", "symmetric_hann", "imag_sign", "f32_trig", "bf16_operands", "pad_columns", "no_eps",
           "no_norm_eps", "legacy_transposed")


def _to_bf16(x):
    return G._to_bf16(np.ascontiguousarray(x, dtype=np.float32))


def _basis32(n_fft, mutant=None):
    if mutant == "symmetric_hann":
        return basis64(n_fft, hann="symmetric").astype(np.float32)
    if mutant == "imag_sign":
        return basis64(n_fft, sign=1.0).astype(np.float32)
    if mutant == "f32_trig":                              # cos, sin and Hann in float32, the phase 2 pi f k / N unreduced
        f32 = np.float32
        k, f = np.arange(n_fft, dtype=f32)[:, None], np.arange(n_fft // 2 + 1, dtype=f32)[None, :]
        ang = f32(2.0 * np.pi) * (f * k) / f32(n_fft)
        w = f32(0.5) - f32(0.5) * np.cos(f32(2.0 * np.pi) * k / f32(n_fft))
        W = np.empty((n_fft, 2 * (n_fft // 2 + 1)), dtype=f32)
        W[:, 0::2], W[:, 1::2] = w * np.cos(ang), -w * np.sin(ang)
        assert W.dtype == f32 and ang.dtype == f32
        return W
    W = basis64(n_fft).astype(np.float32)
    return _to_bf16(W) if mutant == "bf16_operands" else W


def _chain(A, W):
    """every element as ONE sequential float32 chain over k (product rounded, then added)"""
    acc, tmp = np.zeros((A.shape[0], W.shape[1]), dtype=np.float32), np.empty((A.shape[0], W.shape[1]), dtype=np.float32)
    A = np.asfortranarray(A)
    for k in range(A.shape[1]):
        np.multiply(A[:, k:k + 1], W[k][None, :], out=tmp)
        acc += tmp
    return acc


def twin_spectrum(wave, n_fft, hop, T, order="numpy", mutant=None):
    """(B T, 2F) float32"""
    A = frames_of(np.asarray(wave, dtype=np.float32), n_fft, hop, T, offset=1 if mutant == "frame_offset" else 0,
                  next_row=mutant == "pad_next_row")
    if mutant == "bf16_operands":
        A = _to_bf16(A)
    W = _basis32(n_fft, mutant)
    return _chain(A, W) if order == "chain" else A @ W


def twin_features(spec, what, cfg, mutant=None):
    """the epilogues of stft.hip in float32 on a (M, 2F) float32 spectrum (logf taken as correctly rounded)"""
    re, im = spec[:, 0::2], spec[:, 1::2]
    pw = re * re + im * im
    if what == "power":
        return pw
    x = pw if mutant == "no_eps" else pw + np.float32(cfg["eps"])
    with np.errstate(divide="ignore"):
        v = np.log(x.astype(np.float64)).astype(np.float32)
    if what == "log":
        return v
    den = cfg["std"] if mutant == "no_norm_eps" else cfg["std"] + np.float32(cfg["norm_eps"])
    with np.errstate(divide="ignore", invalid="ignore"):
        return ((v - cfg["mean"]) / den).astype(np.float32)


def make_twin(order="numpy", mutant=None):
    assert mutant is None or mutant in MUTANTS

    def impl(what, wave, cfg):
        N, hop = cfg["n_fft"], cfg["hop"]
        B, L = wave.shape
        F = N // 2 + 1
        if what == "center":
            x = wave[0]
            if cfg["pad"] and end_pad(L, N, hop, cfg["fs"]):
                x = np.concatenate([x, np.zeros(hop, dtype=np.float32)])
            wave, cfg = np.pad(x, N // 2, mode="reflect")[None], dict(cfg, pad=False)
            what, L = "legacy", wave.shape[1]
        T = n_frames(L, N, hop, cfg["pad"], cfg["fs"])
        spec = twin_spectrum(wave, N, hop, T, order, mutant)
        if what == "complex":
            return spec.reshape(B, T, F, 2)
        if what == "legacy":
            assert B == 1
            out = spec.reshape(T, F, 2)
            return np.ascontiguousarray(out if mutant == "legacy_transposed" else out.transpose(1, 0, 2)).reshape(F, T, 2)
        if what == "workspace":
            S = np.zeros((B * T, spectrum_ld(N)), dtype=np.float32)
            S[:, :2 * F] = spec
            if mutant == "pad_columns":
                S[:, 2 * F:] = spec[:, :2]
            return S
        return twin_features(spec, "log" if what == "lps" else what, cfg, mutant).reshape(B, T, F)
    return impl
