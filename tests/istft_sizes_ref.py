"""The cases of tests/test_istft_sizes_gpu.py and tests/test_istft_sizes_cpu.py: the masked inverse STFT, its adjoint and
the SI-SDR loss at the sizes where their kernels change behaviour -- past one trip of the grid-stride loops, past the
GEMM rows the small tests reach, past one stride of the loss's single workgroup.  Every reference and every bound is the
one of tests/istft_ref.py and tests/sisdr_ref.py, unchanged; this module only builds the inputs (once per process), states
the forward rule of ``test_istft_gpu._check_row`` for a whole batch, and emulates a kernel that stops after one trip.

A plain module: no fixtures, nothing read from outside the repository."""
import functools

import numpy as np

import istft_ref as R
import score_ref
import sisdr_ref as S

# One trip of a grid-stride loop launched on frames::grid1 (csrc/frames.h): at most 4096 workgroups of 256 threads.
# overlap_add, overlap_add_adjoint, mask_gradient and idft_basis (csrc/istft.hip) take element i >= TRIP in a later trip.
TRIP = 4096 * 256

# 16 ragged rows at 1024 / 256: B T = 4160 GEMM rows (33 x 8 tiles of 128 x 128), pitch 67 328 (66 304 centred), so that
# B pitch = 1 077 248 (1 060 864) > TRIP and the second trip of overlap_add lies in row 15, which is a full row.
FRAMES = (260, 131, 1, 2, 77, 260, 200, 260, 260, 259, 260, 5, 260, 260, 130, 260)
N_FFT, HOP = 1024, 256
LONG = ((64, 16, 65600), (1024, 256, 4100))          # one utterance of L = 1 049 648 and of L = 1 050 368 samples
CHAIN_LENGTHS = tuple([48000] * 14 + [30000, 47000])   # B T F = 16 x 185 x 513 = 1 518 480 elements of mask_gradient


# ------------------------------------------------------------------------------------------------ the forward
@functools.lru_cache(maxsize=None)
def forward_case(n_fft, hop, frames, center=False, mode=0, seed=0):
    """A ragged batch for ``ops.istft``: random unit-peak spectra with NaN in the padding frames, for ``mode`` 2 logits with
    NaN in the padding too.  Per row the float64 numerator and window sum of squares of its (float64-masked) spectrum over
    the row's own natural length, the float32 GEMM form ``y32`` on the same spectrum and its ``E_cpu32``."""
    rng = np.random.default_rng(seed)
    B, T, F = len(frames), max(frames), n_fft // 2 + 1
    spec = np.full((B, T, F, 2), np.nan, dtype=np.float32)
    logits = np.full((B, T, F), np.nan, dtype=np.float32) if mode == 2 else None
    natural = [R.istft_length(nf, n_fft, hop, center) for nf in frames]
    rows = []
    for b, nf in enumerate(frames):
        Sb = R.random_spectrum(rng, nf, n_fft)
        spec[b, :nf, :, 0], spec[b, :nf, :, 1] = Sb.real, Sb.imag
        S64 = Sb.astype(np.complex128)
        if mode == 2:
            logits[b, :nf] = rng.standard_normal((nf, F)) * 2.0
            S64 = S64 * (1.0 / (1.0 + np.exp(-logits[b, :nf].astype(np.float64))))
        if natural[b] == 0:                                          # (one centred frame: nothing is left of it)
            rows.append(None)
            continue
        _, num, wss = R.istft64(S64, n_fft, hop, center=center, length=natural[b])
        y32 = R.istft32_gemm(S64, n_fft, hop, center=center, length=natural[b])
        rows.append(dict(num=num, wss=wss, y32=y32, e32=R.weighted_error(y32, num, wss)[0]))
    return dict(n_fft=n_fft, hop=hop, frames=list(frames), center=center, mode=mode, spec=spec, logits=logits, natural=natural,
                pitch=max(natural), rows=rows)


def yardstick(case):
    """(B, pitch) float32: the float32 GEMM form of every row, zero behind the row's natural length"""
    out = np.zeros((len(case["frames"]), case["pitch"]), dtype=np.float32)
    for b, r in enumerate(case["rows"]):
        if r is not None:
            out[b, :case["natural"][b]] = r["y32"]
    return out


def check_forward(out, case, report=None, name="istft"):
    """``test_istft_gpu._check_row``'s rule on every row of ``out`` (B, pitch): the numerator-weighted error
    ``|y wss64 - num64|`` of every sample within ``FACTOR x E_cpu32`` of the same row, and exact zeros behind the row's
    natural length.  Returns the largest E / E_cpu32."""
    out = np.asarray(out)
    assert out.shape == (len(case["frames"]), case["pitch"]), (out.shape, case["pitch"])
    assert np.isfinite(out).all(), name + ": non-finite values"
    worst = 0.0
    for b, r in enumerate(case["rows"]):
        nat = case["natural"][b]
        behind = out[b, nat:]
        assert not behind.any() and not np.signbit(behind).any(), "%s: row %d is not zero from sample %d" % (name, b, nat)
        if r is None:
            continue
        e, got, ref = R.weighted_error(out[b, :nat], r["num"], r["wss"])
        assert r["e32"] > 0
        print("istft: %-44s E = %.3e  E_cpu32 = %.3e  ratio %.2f" % ("%s row %d (%d frames)" % (name, b, case["frames"][b]),
                                                                    e, r["e32"], e / r["e32"]))
        if report is not None:
            report("%s row %d" % (name, b), got, ref, R.FACTOR * r["e32"])
        assert e <= R.FACTOR * r["e32"], "%s row %d: E = %.3e above %g x E_cpu32 = %.3e" % (name, b, e, R.FACTOR, R.FACTOR * r["e32"])
        worst = max(worst, e / r["e32"])
    return worst


def past_trip(a):
    """the elements of ``a`` a grid-stride loop over ``a.size`` elements reaches only after its first trip"""
    return np.asarray(a).reshape(-1)[TRIP:]


def reference_past_trip(case, b):
    """float64 numerator of row b at the samples whose flat index b pitch + s lies at or beyond TRIP (they are all
    within the row's natural length, or the assertion fails)"""
    first = max(0, TRIP - b * case["pitch"])
    assert first < case["natural"][b], (first, case["natural"][b])
    return case["rows"][b]["num"][first:]


# ------------------------------------------------------------------------------------------------ a kernel of one trip
def stops_after_one_trip(y32):
    """what a grid-stride kernel gives that never takes a second trip, on a zeroed output: ``y32`` with every element of
    flat index >= TRIP zero"""
    out = np.array(y32, copy=True)
    out.reshape(-1)[TRIP:] = 0
    return out


def second_trip_off_by(y32, shift):
    """the second trip computed from an index that is ``shift`` elements off (one batch row, one GEMM row, one frame):
    element i >= TRIP holds the value of element i - shift"""
    out = np.array(y32, copy=True)
    flat, src = out.reshape(-1), np.asarray(y32).reshape(-1)
    assert 0 < shift <= TRIP
    flat[TRIP:] = src[TRIP - shift:src.size - shift]
    return out


# ------------------------------------------------------------------------------------------------ the adjoint
def adjoint_case(which):
    """A: logits (mode 2), not centred.  B: a mask (mode 1), centred, a non-unit scale per row and lengths below the
    natural ones on rows 6 and 15 -- row 15's cut at 60 000 lies inside the second trip of overlap_add_adjoint, which
    starts at q[15][38 656]."""
    if which == "A":
        return S.cached_istft_case(N_FFT, HOP, FRAMES, 2, False, 41)
    nat = [R.istft_length(nf, N_FFT, HOP, True) for nf in FRAMES]
    nat[6], nat[15] = 40000, 60000
    scale = tuple(0.5 + 0.125 * b for b in range(len(FRAMES)))
    return S.cached_istft_case(N_FFT, HOP, FRAMES, 1, True, 42, lengths=tuple(nat), scale=scale)


def adjoint_with_q_of_one_trip(case):
    """The float32 yardstick of dmask when overlap_add_adjoint stops after one trip: q is zero from flat index TRIP on, which
    is the same as a cotangent that is zero from there on.  Only the last batch row holds such samples; its dmask is
    recomputed, the others are the yardstick's."""
    B, T = case["mask"].shape[:2]
    Lq = (T - 1) * case["hop"] + case["n_fft"]
    b = B - 1
    assert b * Lq < TRIP < B * Lq
    first = TRIP - b * Lq - case["start"]                      # first sample of dout[b] whose q lies in the second trip
    assert 0 < first < min(case["lengths"][b], case["dout"].shape[1])
    dout = case["dout"][b:b + 1].copy()
    dout[0, first:] = 0
    one = dict(case, frames=case["frames"][b:], lengths=case["lengths"][b:], spec=case["spec"][b:], mask=case["mask"][b:], dout=dout,
               scale=None if case["scale"] is None else case["scale"][b:])
    out = case["y32"].copy()
    out[b] = S.dmask_closed(one, np.float32)[0]
    return out


@functools.lru_cache(maxsize=None)
def chain_case():
    return S.chain_case(N_FFT, HOP, list(CHAIN_LENGTHS), seed=43)


# ------------------------------------------------------------------------------------------------ the loss over many rows
LOSS_B, LOSS_HEAD, LOSS_TAIL = 300, 24, 36
LOSS_EMPTY_WINDOW, LOSS_ZERO_LENGTH, LOSS_LONG = 270, 280, 290       # planted rows, all at indices >= 256


@functools.lru_cache(maxsize=None)
def loss_case(chunk):
    """300 rows of 300 ... 699 samples (``300 + (7 i) % 400``), one of ``chunk + 77`` (``chunk``: ops.SCORE_CHUNK), one whose
    window is empty and one of length 0, NaN behind the lengths.  Signals as in tests/test_score_gpu.py: s_hat = 0.7 s + g n
    + e, drawn -- next seed on a miss, judged by the float64 reference alone -- so that the three ratios of the whole row
    and the SI-SDR of its window lie in [-10, 60] dB.  Holds ``check_sisdr``'s case and the float64 ratios per row."""
    lengths = [300 + (7 * i) % 400 for i in range(LOSS_B)]
    lengths[LOSS_EMPTY_WINDOW], lengths[LOSS_ZERO_LENGTH], lengths[LOSS_LONG] = 40, 0, chunk + 77
    L = max(lengths)
    est, ref, noise = (np.full((LOSS_B, L), np.nan, dtype=np.float32) for _ in range(3))
    want = np.full((LOSS_B, 3), np.nan)
    gains, arts = (1.0, 0.1, 1e-2), (0.0, 20.0, 40.0)
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        for seed in range(100):
            e, s, v = score_ref.mix(np.random.default_rng([n, b, seed]), n, gains[b % 3], arts[(b // 3) % 3])
            r = np.array(score_ref.energy_ratios(e, s, v))
            lo, hi = LOSS_HEAD, n - LOSS_TAIL
            w = score_ref.energy_ratios(e[lo:hi], s[lo:hi])[0] if hi > lo else 0.0
            if np.all((r >= -10.0) & (r <= 60.0)) and -10.0 <= w <= 60.0:
                break
        else:
            raise AssertionError("no draw for row %d" % b)
        est[b, :n], ref[b, :n], noise[b, :n], want[b] = e, s, v, r
    case = dict(est=est, ref=ref, noise=noise, lengths=lengths, head=LOSS_HEAD, tail=LOSS_TAIL, ratios64=want)
    case["ref64"] = S.sisdr64(est, ref, lengths, LOSS_HEAD, LOSS_TAIL)
    return case
