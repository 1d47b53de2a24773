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


# ------------------------------------------------------------------ cases aimed at the launch shapes of csrc/target.hip
# What the builders below assume of the kernels; tests/test_targets_cpu.py reads each back from the source text.
FS = 16e3
WG = 256                    # threads of every workgroup in target.hip (__launch_bounds__(256))
SEGS_PER_WAVE = 8           # segment_energy: 4 waves x 8 segments per workgroup
MAX_ROWS = 8                # spectrum_max: spectrum rows of one workgroup (a slab)
CAP_MASK = 8192             # grid_cap of ibm_mask and noise_aware_mask: 8192 * 256 threads x 4 outputs per trip
CAP_MASK_STRIDED = 4096     # grid_cap of ibm_mask_strided: 4096 * 256 threads x 4 outputs per trip
CAP_MAX_STRIDED = 1024      # grid_cap of spectrum_max_strided: 1024 * 256 threads x 1 bin per trip
MASK_TRIP = CAP_MASK * WG * 4                    # 8,388,608 outputs
MASK_STRIDED_TRIP = CAP_MASK_STRIDED * WG * 4    # 4,194,304 outputs
MAX_STRIDED_TRIP = CAP_MAX_STRIDED * WG          # 262,144 bins


def trips(n, per_trip):
    return -(-n // per_trip)


def framing(n_fft, hop):
    """wlen_sec / hop_percent that give (n_fft, hop) back through the reference's int() conversions"""
    return dict(fs=FS, wlen_sec=n_fft / FS, hop_percent=hop / n_fft)


def vad_signal(n, seed, quiet_at, width, level=1.0, tail=0):
    """n float32 samples whose frame energies span several decades: white noise under a piecewise-linear log-amplitude
    envelope (knots in -2.2 .. 0 decades) with a V-shaped quiet stretch down to -3.3 decades at sample ``quiet_at``, 1.8
    decades up over ``width`` samples on each side: about 0.85 / 1.8 of the stretch lies under the VAD threshold of
    10**1.7 times the smallest energy.  ``tail`` > 0 drops the last ``tail`` samples by another 6 dB, so the quietest
    frame is one of those that lie wholly inside them."""
    rng = np.random.default_rng(seed)
    knots = max(4, n // 700)
    i = np.arange(n)
    env = np.interp(i, np.linspace(0, n - 1, knots), rng.uniform(-2.2, 0.0, knots))
    env = np.minimum(env, -3.3 + 1.8 * np.abs(i - quiet_at) / width)
    x = rng.standard_normal(n) * 10.0 ** env
    if tail:
        x[n - tail:] *= 10.0 ** -0.3
    return (level * x).astype(np.float32)


SPIKE = 0.5


def spike_signal(n, seed, spikes):
    """n float32 samples: white noise of 1e-3 and single samples of +-0.5 at ``spikes``.  A frame of up to 1024 noise samples
    has an energy of about 1e-3, the VAD threshold is 10**1.7 times the smallest of them and one spike adds 0.25: a frame's
    label is 1 exactly when the samples summed for it hold a spike, so a kernel that skips or adds single samples changes
    the labels of the frames whose only spike lies there."""
    rng = np.random.default_rng(seed)
    x = 1e-3 * rng.standard_normal(n)
    spikes = np.asarray([p for p in spikes if 0 <= p < n], dtype=np.int64)
    x[spikes] = SPIKE * rng.choice([-1.0, 1.0], len(spikes))
    return x.astype(np.float32)


def _scalar_store_row():
    """case 2: the last 53 samples (all that frame 1026 reads besides its end pad) are the quietest, and 32 loud samples
    just before them make frames 1022 .. 1025 ones: the last trip of the scalar store loop writes 1, 1, 0"""
    x = vad_signal(16469, 2, 16469, 9000, tail=53)
    x[16384:16416] = 0.1 * (-1.0) ** np.arange(32)
    return x


def _every(period, phase, n_blocks):
    return [j for j in range(n_blocks) if j % period == phase]


def vad_cases():
    """name -> dict(n_fft, hop, rows: list of float32 signals, T: their frame counts as run, center: the pad modes to run
    when the case is centred).  One call of ops.speech_targets per case (and pad mode); every row is checked against
    vad_energy of that row alone."""
    c = {}
    # 1: T = 1028 at hop 16: five trips of vad_decide's minimum loop (256 frames each), two of its float4 store loop
    #    (1024 frames each); the quiet stretch sits at frame 900, which only the fourth trip of the minimum loop reads
    c["vec_store_T1028"] = dict(n_fft=64, hop=16, rows=[vad_signal(16485, 1, 900 * 16, 3300)], T=[1028])
    # 2: T = 1027: the scalar store loop (T % 4 != 0), five trips; the quietest frame is the last one, and the last trip
    #    of the store loop (frames 1024 .. 1026) writes both labels
    c["scalar_store_T1027"] = dict(n_fft=64, hop=16, rows=[_scalar_store_row()], T=[1027])
    # 3: n_fft % hop != 0: the whole-frame form (R = 1, seg = 1024: four trips of the k loop), T = 257 > 256; with L % 4 == 0
    #    the float4 loads are on and hop = 307 makes (s0 & 3) == 0 hold for every fourth segment only.  A spike is the last
    #    sample of every frame t = 8 m + 1 (start % 4 == 3): frames t .. t + 3 hold it at in-frame index 1023, 716, 409 and
    #    102, one in each trip of the k loop, and frame t loses it when its loads are taken from an aligned address
    spikes = [307 * t + 1023 for t in range(1, 257, 8)]
    c["whole_frame_vec"] = dict(n_fft=1024, hop=307, rows=[spike_signal(79400, 3, spikes)], T=[257])
    c["whole_frame_scalar"] = dict(n_fft=1024, hop=307, rows=[spike_signal(79402, 4, spikes)], T=[257])
    # 4: the guarded last quad: seg % 4 == 2 in the whole-frame form (1002) and in the hop-block form (seg = hop = 250).
    #    Whole frames: a spike at 250 j (+1) is the frame's sample 1000 (1001) for frame j - 4 and one of the first 1000 for
    #    frames j - 3 .. j; a spike at 250 j + 2 (+3) lies just behind frame j - 4, where an unguarded quad would read it
    spikes = [250 * j + (j // 12) % 2 for j in _every(12, 0, 96)] + [250 * j + 2 + (j // 12) % 2 for j in _every(12, 6, 96)]
    c["ragged_quad_whole_frame"] = dict(n_fft=1002, hop=250, rows=[spike_signal(24000, 5, spikes)], T=[93])
    #    Hop blocks: a spike in sample 248 (249) of block j, and one in sample 0 (1) of other blocks, which an unguarded
    #    quad of the block before would add to frame j - 4
    spikes = [250 * j + 248 + (j // 12) % 2 for j in _every(12, 0, 96)] + [250 * j + (j // 12) % 2 for j in _every(12, 6, 96)]
    c["ragged_quad_hop_block"] = dict(n_fft=1000, hop=250, rows=[spike_signal(24000, 6, spikes)], T=[93])
    # 5: hop-block form with seg = 512 > 256: two trips of the k loop, R = 2 blocks per frame; spikes in the second half of
    #    every sixth block and in the first half of the blocks between them
    spikes = [512 * j + 300 + 50 * (j % 4) for j in _every(6, 0, 79)] + [512 * j + 100 for j in _every(6, 3, 79)]
    c["hop_block_seg512"] = dict(n_fft=1024, hop=512, rows=[spike_signal(40000, 7, spikes)], T=[78])
    # 6: centred and ragged: row 0 fills the pitch and gets the end pad, so its reflection point and its zeros lie past
    #    the row (n > nread); row 1 is a whole number of hops by the reference's test (no end pad), row 2 is not.
    #    Sample 32 reaches frame 0 only through the reflection, and sample n - 33 the last frame of a row without end pad;
    #    sample L - 33 of row 0 (end-padded) reaches its last frame only if the reflection ignores the pad; sample 5 of
    #    row 1 lies where row 0's end pad would be read if the row's width did not bound it
    inner = list(range(200, 1800, 128))
    c["centred_ragged"] = dict(n_fft=64, hop=16, center=("reflect", "constant"),
                               rows=[spike_signal(2005, 8, [32, 2005 - 33] + inner),
                                     spike_signal(1024, 9, [5, 1024 - 33] + [p for p in inner if p < 900]),
                                     spike_signal(1531, 10, [32] + [p for p in inner if p < 1400])],
                               T=[127, 65, 97])
    #    row 2 has an end pad and lies inside the pitch: nothing reaches its last frame through the reflection alone, but
    #    its last sample is summed twice there (not so when mirrored about the length, or not at all), and at 0.0332 it
    #    passes the threshold only so
    c["centred_ragged"]["rows"][2][1531 - 1] = 0.0332
    # 7: a long and a short row in one call, 100x apart in level: vad_decide's workgroups run five trips and one
    c["long_and_short"] = dict(n_fft=64, hop=16, rows=[vad_signal(16485, 11, 850 * 16, 3300, level=0.01),
                                                       vad_signal(3003, 12, 1500, 600, level=1.0)], T=[1028, 185])
    return c


LATE_MIN = {"vec_store_T1028": 0, "scalar_store_T1027": 0, "long_and_short": 0}    # case -> row whose minimum lies past frame 256


def vad_reference(case, row, pad_mode=None):
    """(E float64 (T,), coefficient) of one row of a case, alone"""
    kw = framing(case["n_fft"], case["hop"])
    return vad_energy(case["rows"][row], center=pad_mode is not None, pad_mode=pad_mode or "reflect", **kw)


def segment_model(case, keep=None, over=0, aligned=False):
    """E (T,) of row 0 of a case that is not centred, summed as segment_energy does (whole frames, or R hop-sized blocks per
    frame) -- with one mistake when asked: ``keep`` (seg,) bool drops samples of every segment, ``over`` adds that many
    samples behind every segment (an unguarded last quad), ``aligned`` starts every whole frame at its start rounded down
    to a multiple of 4 (a float4 load taken without the alignment test).  With no mistake this is vad_energy."""
    n_fft, hop = case["n_fft"], case["hop"]
    fr = frames_of(case["rows"][0], center=False, **framing(n_fft, hop))
    T = len(fr)
    y = np.zeros((T - 1) * hop + n_fft + 8)
    y[np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]] = fr
    blocks = n_fft // hop if n_fft % hop == 0 else 1
    seg = hop if blocks > 1 else n_fft
    keep = np.ones(seg, bool) if keep is None else keep
    E = np.zeros(T)
    for r in range(blocks):
        start = np.arange(T) * hop + r * seg
        if aligned:
            start = start - start % 4
        E += (y[start[:, None] + np.flatnonzero(keep)[None, :]] ** 2).sum(axis=1)
        for q in range(over):
            E += y[start + seg + q] ** 2
    return E


def centred_model(case, b, mode, reflect_at="own", bounded=True):
    """E (T_b,) of row b of a centred case inside its zero-padded batch, sample by sample as sample_at of target.hip reads
    it: the padded index j is sample s = j - n_fft/2; 'reflect' mirrors s < 0 about 0 and s >= n about n - 1, n being the
    row's length after its end pad; a sample is read when 0 <= s < min(n, the batch's width), else it is zero.  The
    mistakes: ``reflect_at`` 'widest' mirrors every row about the widest row's n, 'length' about the row's length
    without its end pad; ``bounded`` False reads up to n, which behind the batch's width is the next row."""
    n_fft, hop = case["n_fft"], case["hop"]
    off = n_fft // 2
    wave, lens = batch_of(case["rows"])
    pitch = wave.shape[1]
    flat = np.concatenate([wave.reshape(-1).astype(np.float64), np.zeros(pitch)])

    def padded(L):
        v = L / FS / (n_fft / FS) / (hop / n_fft)
        return L + (hop if math.ceil(v) != int(v) else 0)
    n = padded(lens[b])
    T = 1 + (n + 2 * off - n_fft) // hop
    at = {"own": n, "widest": max(padded(L) for L in lens), "length": lens[b]}[reflect_at]
    s = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :] - off
    if mode == "reflect":
        s = np.where(s < 0, -s, s)
        s = np.where(s >= at, 2 * (at - 1) - s, s)
    live = (s >= 0) & (s < (min(n, pitch) if bounded else n))
    v = np.where(live, flat[b * pitch + np.clip(s, 0, 2 * pitch - 1)], 0.0)
    return (v * v).sum(axis=1)


def batch_of(rows):
    """(float32 (B, max len) zero-padded, lengths)"""
    lens = [len(r) for r in rows]
    wave = np.zeros((len(rows), max(lens)), np.float32)
    for b, r in enumerate(rows):
        wave[b, :lens[b]] = r
    return wave, lens


# ---- IBM from the waveform: one batch past ibm_mask's first grid-stride trip
IBM_FRAMES = (403, 1210, 2005, 4101)        # T_b % 8 = 3, 2, 5, 5: every row ends in a partial slab of spectrum_max; each
#                                             is a whole number of hops by the reference's float test too: no end pad
IBM_LEVELS = (1.0, 100.0, 0.01, 1.0)
IBM_LATE_PEAK = (1, 3)                      # rows whose loudest bin lies in their last live frame


def ibm_signal(T, seed, level, late_peak):
    """(T - 1) * 256 + 1024 float32 samples (a whole number of hops): 40 harmonics of a slowly gliding pitch under a slow
    envelope of 1.5 decades, each harmonic with a slow gain of its own, plus noise 60 dB under the loudest harmonic.
    ``late_peak``: a louder tone over the last 1024 samples, which only the last frame holds in full."""
    rng = np.random.default_rng(seed)
    n = (T - 1) * 256 + 1024
    t = np.arange(n) / FS
    f0 = 140.0 + 40.0 * np.sin(2 * np.pi * t / 3.1 + rng.uniform(0, 6.28))
    phase = 2 * np.pi * np.cumsum(f0) / FS
    env = 10.0 ** (-0.75 + 0.75 * np.sin(2 * np.pi * t / 1.7 + rng.uniform(0, 6.28)))
    x = np.zeros(n)
    coarse = t[::256]
    for k in range(1, 41):
        gain = 10.0 ** (-0.5 + 0.5 * np.sin(2 * np.pi * coarse / rng.uniform(0.8, 2.5) + rng.uniform(0, 6.28))) / k ** 0.5
        x += np.interp(t, coarse, gain) * np.sin(k * phase + rng.uniform(0, 6.28))
    x = env * x + 1e-3 * rng.standard_normal(n)
    if late_peak:
        x[n - 1024:] += 2.0 * np.sin(2 * np.pi * 40 * np.arange(1024) / 1024)
    return (level * x).astype(np.float32)


def ibm_rows():
    """the four rows, the longest last: ibm_mask's second trip (outputs from MASK_TRIP on) then lies in live frames"""
    return [ibm_signal(T, 20 + b, IBM_LEVELS[b], b in IBM_LATE_PEAK) for b, T in enumerate(IBM_FRAMES)]


# ---- IBM from a given spectrum: past the first trip of both strided kernels
SPEC_F, SPEC_T = 513, 8200
SPEC_PEAK = (400, 1234)                     # (f, t) of the planted maximum: flat index f * T + t = 3,281,234


def strided_spectrum(seed=31):
    """complex64 (513, 8200): magnitudes over four decades and one planted maximum far behind the bins that
    spectrum_max_strided reads in its first two trips; vad (8200,) of zeros and ones"""
    rng = np.random.default_rng(seed)
    shape = (SPEC_F, SPEC_T)
    mag = 10.0 ** rng.uniform(-3, 1, shape).astype(np.float32)
    S = (rng.standard_normal(shape, dtype=np.float32) + 1j * rng.standard_normal(shape, dtype=np.float32)) * mag
    S = S.astype(np.complex64)
    S[SPEC_PEAK] = 90.0 - 60.0j
    vad = (rng.random(SPEC_T) < 0.6).astype(np.float32)
    return S, vad


def ibm_exact(S, eps=1e-8, ibm_threshold=50, max_power=None):
    """ibm_mask_strided restated in float64 in the kernel's order, from a complex64 spectrum -> (mask bool, undecided
    bool).  P = re^2 + im^2 (the squares of float32 values are exact in double, their sum is rounded once, fused or not),
    tau = (sqrt(max P) + eps) * coef - eps with the float32 eps of the descriptor, bit = tau < 0 or P > tau^2.  The
    device may fuse the product and the subtraction of tau, which moves its last bit: bins with |P - tau^2| <= 1e-12 tau^2
    are undecided.  ``max_power`` replaces max P (what a kernel that lost a trip's maximum would use)."""
    re, im = S.real.astype(np.float64), S.imag.astype(np.float64)
    P = re * re + im * im
    e = np.float64(np.float32(eps))
    coef = np.power(10, np.float64(-ibm_threshold / 20.0))
    tau = (np.sqrt(P.max() if max_power is None else max_power) + e) * coef - e
    return (tau < 0) | (P > tau * tau), np.abs(P - tau * tau) <= 1e-12 * tau * tau


# ---- noise-aware masks: one call past noise_aware_mask's first trip
NA_B, NA_T = 2, 8201


def noise_aware_row(b, seed=41):
    """(X, N) complex64 (8201, 513) of row b: magnitudes over four decades, as in the small cases of test_noise_aware_gpu"""
    rng = np.random.default_rng(seed + b)
    shape = (NA_T, 513)

    def one():
        mag = 10.0 ** rng.uniform(-3, 1, shape).astype(np.float32)
        return ((rng.standard_normal(shape, dtype=np.float32) + 1j * rng.standard_normal(shape, dtype=np.float32)) * mag).astype(np.complex64)
    return one(), one()
