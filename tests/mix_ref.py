"""Float64 reference of the SNR mix (csrc/mix.hip, include/avvad.h avvad_mix), the cases the CPU and GPU tests share, and
the assertions, which take the implementation as a callable -- the pattern of score_ref.py and head_ref.py.

Semantics: row b has speech s = clean[b][:len_b] and noise n[i] = clip[(start + i) mod len(clip)];
Es = sum s^2, En = sum n^2 over i < len_b in double; g = float32(sqrt(Es / (En 10^(snr_db / 10)))), 0 for a degenerate row
(len_b == 0, Es == 0 or En == 0); noise_out = g n, noisy = s + g n, exact zeros from len_b to L.

An implementation is ``impl(case) -> {"noisy" (B, L) f32, "noise" (B, L) f32, "gain" (B,) f32, "energies" (B, 2) f64,
"peak" (B,) f32}`` of numpy arrays.  A case: ``clean`` (B, L) float32 (finite garbage behind each length, which must not
reach a result), ``lengths``, ``clips`` (list of float32 arrays), ``clip``, ``start``, ``snr_db`` (lists of B).

Bounds of ``check`` -- each follows from the arithmetic, not from a run:
  energies  1e-12 relative to float64: the squares are exact in double (24-bit significands), only the additions round.
            All terms are >= 0, so a sum is off by at most d 2^-53 of itself, d the longest chain of additions a term
            passes through: at most 16 + 6 + 3 + 4 = 29 in the kernel (per lane, butterfly, waves, chunks) and about as
            many in numpy's pairwise sum -- some 1e-14 between the two, far inside the bound.
  gain      2^-23 relative to sqrt(Es64 / (En64 ratio)): one rounding to float (2^-24) plus the energies' 1e-12.
  noisy     |noisy - (s + g n)| <= 2^-24 (|g n| + |s + g n|) in float64 with the implementation's OWN g: a rounded
            product then a rounded sum, or one fused rounding, and nothing looser.
  noise     == float32(g n) exactly (the product of two floats is exact in double: one rounding).
  SNR       10 log10(sum s^2 / sum noise^2) within 1e-5 dB of the request (g's rounding moves it by at most
            20 log10(1 + 2^-24) = 5.2e-7 dB, the products' roundings average out below that).
  peak      == max |noisy| of the returned row, bit for bit; zeros from len_b to L in noisy and noise.

Cases: "ragged" (the 12 rows of ROWS), "wide" (B = 33) and "wide70" (B = 70: mix_gain takes one thread per row in
workgroups of 64, so rows 64 to 69 -- ROWS[4..9], none degenerate -- are the second workgroup's, which nothing below
B = 65 launches).  The mutant "gain_past_64_rows" is that second workgroup missing; only "wide70" can see it.
"""
import functools

import numpy as np

from avvad import _lib

CHUNK = _lib.MIX_CHUNK   # the rows and clips below lie around the kernel's chunk (AVVAD_MIX_CHUNK, 4096)
EPS24 = 2.0 ** -24
GARBAGE = 3.0            # what clean holds behind each row's length


def noise_segment(clip, start, n):
    """the first n samples of the clip read circularly from start"""
    return clip[(start + np.arange(n, dtype=np.int64)) % clip.size]


def reference(case):
    """per row (Es, En, g64): float64 energies over the row's samples and the unrounded gain (0 for a degenerate row)"""
    out = []
    for b, n in enumerate(case["lengths"]):
        s = case["clean"][b, :n].astype(np.float64)
        v = noise_segment(case["clips"][case["clip"][b]], case["start"][b], n).astype(np.float64)
        es, en = float(np.sum(s * s)), float(np.sum(v * v))
        ratio = float(np.power(10.0, np.float64(case["snr_db"][b]) / 10.0))
        g = float(np.sqrt(es / (en * ratio))) if n > 0 and es > 0 and en > 0 else 0.0
        out.append((es, en, g))
    return out


def _speech(rng, n):
    env = 0.05 + 0.1 * np.abs(np.sin(np.arange(n) / 700.0))
    return (rng.standard_normal(n) * env).astype(np.float32)


def make_case(rows, clips, pad=7):
    """rows: (length, clip, start, snr_db, silent speech?) -> a case with pitch max(length) + pad"""
    rng = np.random.default_rng(20240)
    L = max(r[0] for r in rows) + pad
    clean = np.full((len(rows), L), GARBAGE, dtype=np.float32)
    for b, (n, _, _, _, silent) in enumerate(rows):
        clean[b, :n] = 0.0 if silent else _speech(rng, n)
    return {"clean": clean, "lengths": [r[0] for r in rows], "clips": clips, "clip": [r[1] for r in rows],
            "start": [r[2] for r in rows], "snr_db": [r[3] for r in rows], "L": L}


@functools.lru_cache(maxsize=None)
def clips():
    """lengths 1, 255, CHUNK, 5000, 3 CHUNK + 17, 300, and 6000 with a silent stretch [1000, 3000)"""
    rng = np.random.default_rng(77)
    out = [(rng.standard_normal(n) * 0.05).astype(np.float32) for n in (1, 255, CHUNK, 5000, 3 * CHUNK + 17, 300, 6000)]
    out[0][0] = 0.04
    out[6][1000:3000] = 0.0
    return tuple(out)


LONG = 3 * CHUNK + 17
#        length  clip start   snr   silent speech
ROWS = [(0,      3,   10,    0.0, False),     # an empty row
        (1,      0,    0,    0.0, False),     # one sample of a one-sample clip
        (255,    1,  100,    7.5, False),     # the clip as long as the row, read from its middle
        (4095,   2, 4095,  -20.0, False),     # starts on the clip's last sample
        (4096,   3, 4999,   40.0, False),     # wraps after one sample
        (4097,   3,   17,    0.0, False),     # the same clip at another start
        (LONG,   4,    0,    7.5, False),     # clip == row: never wraps
        (9000,   5,  123,  -20.0, False),     # a 300-sample clip: wraps many times per chunk and across chunk boundaries
        (LONG,   2,    1,   40.0, False),     # a clip of exactly one chunk under four chunks
        (9000,   0,    0,    0.0, False),     # the one-sample clip under three chunks
        (1500,   6, 1200,    7.5, False),     # an all-zero clip segment
        (4097,   3, 2500,    7.5, True)]      # all-zero speech
DEGENERATE = (0, 10, 11)


@functools.lru_cache(maxsize=None)
def ragged_case():
    return make_case(ROWS, clips())


@functools.lru_cache(maxsize=None)
def wide_case():
    """B = 33: the rows above in turn, with the four SNRs going round"""
    snrs = (-20.0, 0.0, 7.5, 40.0)
    rows = [ROWS[i % len(ROWS)][:3] + (snrs[i % 4], ROWS[i % len(ROWS)][4]) for i in range(33)]
    return make_case(rows, clips())


@functools.lru_cache(maxsize=None)
def wide70_case():
    """B = 70: as wide_case, past the 64 rows of one mix_gain workgroup; rows 64 to 69 are ROWS[4..9]"""
    snrs = (-20.0, 0.0, 7.5, 40.0)
    rows = [ROWS[i % len(ROWS)][:3] + (snrs[i % 4], ROWS[i % len(ROWS)][4]) for i in range(70)]
    return make_case(rows, clips())


NAMED = {"ragged": ragged_case, "wide": wide_case, "wide70": wide70_case}


def rows_of(case, rows):
    """the given rows of a case as a case of its own (the same pitch)"""
    sub = dict(case)
    sub["clean"] = case["clean"][list(rows)]
    for k in ("lengths", "clip", "start", "snr_db"):
        sub[k] = [case[k][b] for b in rows]
    return sub


def single_row(case, b):
    """row b of a case as a case of its own (B = 1, the same pitch)"""
    return rows_of(case, [b])


@functools.lru_cache(maxsize=None)
def _reference_of(name):
    return reference(NAMED[name]())


def check(impl, case, ref=None):
    """every bound of the module's docstring on impl(case); returns impl's outputs"""
    got = impl(case)
    ref = ref if ref is not None else reference(case)
    B, L = case["clean"].shape
    noisy, noise, gain, energies, peak = (np.asarray(got[k]) for k in ("noisy", "noise", "gain", "energies", "peak"))
    assert noisy.shape == noise.shape == (B, L) and noisy.dtype == noise.dtype == np.float32
    assert gain.shape == peak.shape == (B,) and gain.dtype == peak.dtype == np.float32
    assert energies.shape == (B, 2) and energies.dtype == np.float64
    for k in ("noisy", "noise", "gain", "energies", "peak"):
        assert np.isfinite(got[k]).all(), "%s is not finite everywhere" % k
    for b, n in enumerate(case["lengths"]):
        es, en, g64 = ref[b]
        s = case["clean"][b, :n]
        v = noise_segment(case["clips"][case["clip"][b]], case["start"][b], n)
        tag = "row %d (len %d, clip %d of %d, start %d, %.1f dB)" % (b, n, case["clip"][b], case["clips"][case["clip"][b]].size,
                                                                    case["start"][b], case["snr_db"][b])
        for q, want in enumerate((es, en)):
            assert abs(energies[b, q] - want) <= 1e-12 * want, "%s: energy %d = %r, float64 %r" % (tag, q, energies[b, q], want)
        g = float(gain[b])
        assert abs(g - g64) <= 2.0 ** -23 * g64, "%s: gain %r, float64 %r" % (tag, g, g64)
        assert not noisy[b, n:].any() and not noise[b, n:].any(), "%s: the tail is not zero" % tag
        if g64 == 0.0:
            assert g == 0.0 and np.array_equal(noisy[b, :n].view(np.int32), s.view(np.int32)) and not noise[b, :n].any(), \
                "%s: a degenerate row must leave the speech alone" % tag
        else:
            gn = g * v.astype(np.float64)
            want = s.astype(np.float64) + gn
            err = np.abs(noisy[b, :n].astype(np.float64) - want)
            bound = EPS24 * (np.abs(gn) + np.abs(want))
            assert (err <= bound).all(), "%s: noisy off by up to %.3g bounds at %d" % (tag, (err / np.maximum(bound, 1e-300)).max(),
                                                                                    int(np.argmax(err - bound)))
            assert np.array_equal(noise[b, :n].view(np.int32), gn.astype(np.float32).view(np.int32)), \
                "%s: noise is not float32(g n)" % tag
            snr = 10.0 * np.log10(np.sum(s.astype(np.float64) ** 2) / np.sum(noise[b, :n].astype(np.float64) ** 2))
            assert abs(snr - case["snr_db"][b]) <= 1e-5, "%s: realised SNR %.7f dB" % (tag, snr)
        want_peak = np.abs(noisy[b]).max() if L else np.float32(0)
        assert peak[b].view(np.int32) == np.float32(want_peak).view(np.int32), "%s: peak %r, max |noisy| %r" % (tag, peak[b], want_peak)
    return got


def check_named(impl, name):
    """``check`` on the shared case ``name`` ("ragged", "wide", "wide70") with its reference computed once"""
    return check(impl, NAMED[name](), _reference_of(name))


MUTANTS = ("no_wrap", "start_ignored", "en_whole_clip", "energies_over_pitch", "snr_over_20", "gain_on_speech",
           "tail_not_zeroed", "noise_without_gain", "gain_through_float16")
LOOP_MUTANTS = ("gain_past_64_rows",)      # rows b >= 64 get g = 0, energies 0 and the speech passed through: "wide70" alone sees it


def standin(case, mutant=None):
    """A float32 numpy implementation of the semantics (float64 energies, one rounded product, one rounded sum); with
    ``mutant`` one of MUTANTS or LOOP_MUTANTS, that mistake built in."""
    assert mutant is None or mutant in MUTANTS + LOOP_MUTANTS
    B, L = case["clean"].shape
    out = {"noisy": np.zeros((B, L), np.float32), "noise": np.zeros((B, L), np.float32), "gain": np.zeros(B, np.float32),
           "energies": np.zeros((B, 2), np.float64), "peak": np.zeros(B, np.float32)}
    for b, n in enumerate(case["lengths"]):
        clip = case["clips"][case["clip"][b]]
        start = 0 if mutant == "start_ignored" else case["start"][b]
        if mutant == "no_wrap":
            v = clip[np.minimum(start + np.arange(n), clip.size - 1)]
        else:
            v = noise_segment(clip, start, n)
        s = case["clean"][b, :n]
        es_src = case["clean"][b] if mutant == "energies_over_pitch" else s
        en_src = clip if mutant == "en_whole_clip" else v
        es = float(np.sum(es_src.astype(np.float64) ** 2))
        en = float(np.sum(en_src.astype(np.float64) ** 2))
        ratio = 10.0 ** (case["snr_db"][b] / (20.0 if mutant == "snr_over_20" else 10.0))
        if mutant == "gain_past_64_rows" and b >= 64:
            es = en = 0.0
        g = np.float32(np.sqrt(es / (en * ratio))) if n > 0 and es > 0 and en > 0 else np.float32(0)
        if mutant == "gain_through_float16":
            g = np.float32(np.float16(g))
        out["gain"][b] = g
        out["energies"][b] = (es, en)
        if mutant == "gain_on_speech":
            out["noise"][b, :n] = v
            out["noisy"][b, :n] = g * s + v if g != 0 else s
        else:
            out["noise"][b, :n] = v if mutant == "noise_without_gain" else g * v
            out["noisy"][b, :n] = s + g * v if g != 0 else s
        if mutant == "tail_not_zeroed":
            out["noisy"][b, n:] = case["clean"][b, n:]
        out["peak"][b] = np.abs(out["noisy"][b]).max()
    return out
