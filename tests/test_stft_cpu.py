"""CPU tests of the STFT oracle (tests/stft_ref.py): the lines of csrc/stft.hip and csrc/frames.h its restatements cite, the
restated plan of every case and the schedules the cases reach together, the frame count of ``ops.n_frames`` against the
float32 restatement of the original over the lengths where its float test decides, the descriptor rule through the library's
host side, every case of tests/test_stft_gpu.py with the float32 twin in the place of the HIP path (in numpy's order and as
one sequential chain), and mutants of that twin which the assertion named for each must reject."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import stft_ref as R

TAG = "cpu32"


def _src(name):
    with open(os.path.join(R.CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------ the restatements against the source
def test_cited_lines_hold():
    lines = {f: _src(f).split("\n") for f in {c[0] for c in R.CITES}}
    for f, n, text in R.CITES:
        assert text in lines[f][n - 1], "%s:%d no longer holds %r: move the citation in stft_ref" % (f, n, text)
    # what the restatements take for granted beyond single lines
    stft, frames = lines["stft.hip"], lines["frames.h"]
    assert "if (x < X && k < K) {" in stft[25] and "static constexpr bool KCONTIG = true;" in stft[15]
    assert "(d->mode == 2 && d->B != 1)" not in "\n".join(stft) and "(mode == 2 && d->B != 1)" in "\n".join(stft)
    assert "return Phase{2.0 * (double)fk / (double)N};" in frames[27]
    assert "w.W = base;" in frames[73]


def test_layout_restated():
    for n_fft, ld in ((1024, 1028), (512, 516), (96, 100), (32, 36), (256, 260), (64, 68)):
        assert R.spectrum_ld(n_fft) == ld
        assert R.ws_spectrum_offset(n_fft) % 64 == 0 and 0 <= R.ws_spectrum_offset(n_fft) - n_fft * ld < 64


def test_cases_reach_what_they_claim():
    """every case against the restated plan, and the schedules, tile counts and shapes the cases reach between them"""
    plans = {name: R.plan_of(name) for name in R.CASES}
    for name, c in R.CASES.items():
        for k, v in c["reach"].items():
            assert plans[name][k] == v, "%s: %s is %r, the case list says %r" % (name, k, plans[name][k], v)
        assert R.case_T(c) >= 1
    for group in (R.IMPULSE, R.ROUNDING):
        assert {plans[n]["schedule"] for n in group} == {"pool", "full", "both"}
    p = plans[R.SCHEDULE_CASE]
    assert p["full_rounds"] >= 1 and p["rem"] > 0 and p["split_tiles"] > 0 and 21000 < p["M"] < 23000
    assert {(R.CASES[n]["n_fft"], R.CASES[n]["hop"]) for n in R.IMPULSE} == set(R.CONFIGS)
    assert {(R.CASES[n]["n_fft"], R.CASES[n]["hop"]) for n in R.ROUNDING} == set(R.CONFIGS)
    Ms = {plans[n]["M"] for n in R.IMPULSE}
    assert {1, 60, 128, 129} <= Ms and any(plans[n]["ntm"] == 3 and R.CASES[n]["B"] == 3 for n in R.IMPULSE)
    # T = 1, n_fft + j hop exactly and +-1, the padded multiple and its neighbour with and without the pad, one second
    for n_fft, hop in R.CONFIGS:
        Ls = {c["L"] for c in R.CASES.values() if (c["n_fft"], c["hop"]) == (n_fft, hop) and c["signal"] == "impulse"}
        assert {n_fft, n_fft + 7 * hop - 1, n_fft + 7 * hop, n_fft + 7 * hop + 1, 16000} <= Ls
    assert R.end_pad(43 * 256, 1024, 256) and not R.end_pad(44 * 256, 1024, 256)
    # the end pad is reached with rows behind the padded one, and the slab of the engine holds every plan
    assert any(c["B"] > 1 and c["pad"] and R.end_pad(c["L"], c["n_fft"], c["hop"]) for c in R.CASES.values())
    assert all(p["G"] * 128 * 128 <= R.G.SLAB_FLOATS for p in plans.values())


def test_impulses_sit_where_indexing_goes_wrong():
    for name in R.IMPULSE:
        c = R.CASES[name]
        B, L, N, hop, T = c["B"], c["L"], c["n_fft"], c["hop"], R.case_T(c)
        seen = set()
        for wave, placed in R.impulse_waves(name):
            assert sorted((b, p) for b, p in zip(*np.nonzero(wave))) == sorted((b, p) for b, p, _ in placed)
            for b in range(B):
                ps = sorted(p for bb, p, _ in placed if bb == b)
                assert all(q - p >= N for p, q in zip(ps, ps[1:])), name
            assert all(abs(a) == 2.0 ** round(np.log2(abs(a))) for _, _, a in placed)
            seen |= {(b, p) for b, p, _ in placed}
        for b in range(B):
            assert (b, 0) in seen and (b, L - 1) in seen and ((T - 1) * hop >= L or (b, (T - 1) * hop) in seen), (name, b)
            assert (T - 1) * hop + N - 1 >= L or (b, (T - 1) * hop + N - 1) in seen, (name, b)
        for m in range(0, B * T, 128):
            b, t = divmod(m, T)
            assert (b, t * hop) in seen and (t * hop + N - 1 >= L or (b, t * hop + N - 1) in seen), (name, m)


# ------------------------------------------------------------------------------------------ the frame count
def _oracle_frames(L, n_fft, hop, fs):
    from oracle import frontend
    wlen_sec, hop_percent = n_fft / fs, hop / n_fft
    assert wlen_sec * fs == int(wlen_sec * fs) and int(wlen_sec * fs) == n_fft and int(hop_percent * n_fft) == hop   # stft_pytorch's check
    return frontend.stft(torch.zeros(L), fs=fs, wlen_sec=wlen_sec, hop_percent=hop_percent, center=False, pad_at_end=True).shape[1]


@pytest.mark.parametrize("n_fft,hop,ks", [(1024, 256, range(4, 401)), (96, 32, range(3, 101))])
def test_n_frames_is_the_originals_frame_count(n_fft, hop, ks):
    """every L in {hop k - 1, hop k, hop k + 1}: ``ops.n_frames`` (and the oracle's restatement) against the frame count of the
    float32 restatement of the original on a zero wave; the exact multiples at which its float test pads are a non-empty set"""
    from avvad import ops
    # a sampling rate at which the original's own check of an integer window length passes, as stft_pytorch requires
    fs = next(f for f in (16e3, 8e3, 48e3, 32e3) if (n_fft / f) * f == int((n_fft / f) * f) and int((n_fft / f) * f) == n_fft)
    padded = []
    for k in ks:
        for L in (hop * k - 1, hop * k, hop * k + 1):
            if L < n_fft:
                continue
            want = _oracle_frames(L, n_fft, hop, fs)
            assert ops.n_frames(L, n_fft, hop, True, fs) == want == R.n_frames(L, n_fft, hop, True, fs), (L, want)
            assert ops.n_frames(L, n_fft, hop, False, fs) == (L - n_fft) // hop + 1 == R.n_frames(L, n_fft, hop, False, fs)
            if L == hop * k and want == (L + hop - n_fft) // hop + 1:
                padded.append(k)
    print("n_fft %d hop %d fs %g: %d of %d exact multiples pad, the first %s" % (n_fft, hop, fs, len(padded), len(ks), padded[:8]))
    assert padded and len(padded) < len(ks)
    if (n_fft, hop, fs) == (1024, 256, 16e3):
        assert padded[:6] == [43, 51, 59, 71, 86, 87]


def test_cases_frame_counts_are_ops_frame_counts():
    from avvad import ops
    for c in R.CASES.values():
        assert ops.n_frames(c["L"], c["n_fft"], c["hop"], c["pad"], c["fs"]) == R.case_T(c)


# ------------------------------------------------------------------------------------------ the descriptor rule (frames.h ok_desc)
def test_descriptor_rule():
    from avvad import _lib as L
    h = L.lib()

    def ok(B, Ls, n_fft, hop, T):
        d = L.StftDesc(B, Ls, n_fft, hop, T, 1e-8)
        need = h.avvad_stft_workspace(C.byref(d))
        p = 0x1000                                            # never dereferenced: a refused descriptor returns first
        if need == 0:
            assert h.avvad_stft(p, p, C.byref(d), 0, p, 1 << 40, None) == -1
            assert h.avvad_stft_complex(p, p, C.byref(d), p, 1 << 40, None) == -1
            assert h.avvad_stft_features(p, p, p, p, C.byref(d), 1e-8, p, 1 << 40, None) == -1
        return need > 0
    assert ok(3, 16000, 1024, 256, 60) and ok(3, 16000, 1024, 256, 59)
    assert not ok(3, 16000, 1024, 256, 61)                    # T one too many: more than the one-hop end pad
    assert ok(1, 1024, 1024, 256, 1) and ok(1, 1024, 1024, 256, 2) and not ok(1, 1024, 1024, 256, 3)
    assert not ok(3, 16000, 1024, 0, 60) and not ok(3, 16000, 1024, -256, 60)
    assert ok(1, 100, 32, 8, 9) and ok(1, 100, 64, 16, 3)     # n_fft = 32 and 64 are accepted
    assert not ok(1, 100, 48, 16, 3) and not ok(1, 100, 16, 4, 3) and not ok(1, 16000, 1000, 250, 4)
    assert not ok(0, 16000, 1024, 256, 60) and not ok(3, 0, 1024, 256, 1) and not ok(3, 16000, 1024, 256, 0)
    assert ok(1, 500, 96, 100, 5) and ok(1, 500, 96, 100, 6) and not ok(1, 500, 96, 100, 7)      # hop > n_fft
    assert h.avvad_stft_workspace(None) == 0
    # mode 2 takes one utterance; modes outside 0 .. 2 are refused; features need both statistics
    d2 = L.StftDesc(2, 16000, 1024, 256, 60, 1e-8)
    p = 0x1000
    assert h.avvad_stft(p, p, C.byref(d2), 2, p, 1 << 40, None) == -1 and h.avvad_stft(p, p, C.byref(d2), 3, p, 1 << 40, None) == -1
    assert h.avvad_stft_features(p, p, None, p, C.byref(d2), 1e-8, p, 1 << 40, None) == -1
    assert h.avvad_stft_features(p, None, p, p, C.byref(d2), 1e-8, p, 1 << 40, None) == -1
    assert h.avvad_stft(p, p, C.byref(d2), 0, p, 64, None) == -2          # a workspace too small


def test_python_layer_refuses_before_any_launch():
    """a host tensor never reaches the library; a mean without a std, a mode-2 batch, a short wave and n_fft = 48 are what
    tests/test_stft_gpu.py refuses with GPU tensors"""
    from avvad import ops
    from avvad._lib import AvvadError
    with pytest.raises(AvvadError):
        ops.stft(torch.zeros(2, 16000))
    with pytest.raises(AvvadError):
        ops.stft_complex(torch.zeros(16000))
    assert ops.n_frames(700, 1024, 256) <= 0 < ops.n_frames(1000, 1024, 256)


# ------------------------------------------------------------------------------------------ the float32 twin passes
# (the impulse tier rounds nothing in any order; the sequential chain of the 22 000-frame case alone would take 25 s)
@pytest.mark.parametrize("name,order", [(n, o) for n in R.IMPULSE for o in ("numpy", "chain") if (n, o) != ("imp-256x64-sched", "chain")])
def test_impulse_tier_holds_for_the_float32_twin(name, order):
    off, total = R.check_impulse(R.make_twin(order), name, tag=TAG + "-" + order)
    assert total > 0 and off == 0             # the twin's basis IS float32(reference): not one ulp of difference


@pytest.mark.parametrize("order", ["numpy", "chain"])
@pytest.mark.parametrize("name", R.ROUNDING)
def test_rounding_tier_is_within_reach_of_float32(name, order):
    fig = R.check_rounding(R.make_twin(order), name, tag=TAG + "-" + order)
    assert 0 < fig["worst"] <= 1
    if R.CASES[name]["features"]:
        fig = R.check_features(R.make_twin(order), name, tag=TAG + "-" + order)
        assert 0 < fig["log"] <= 1 and 0 < fig["std"] <= 1 and 0 < fig["power"] <= 1


def test_unchecked_shares_hold_on_the_reference_alone():
    """0 for the white feature cases, at most 1 % for the tilted one -- and why n_fft 1024 carries no feature case: a white
    spectrum leaves some of its bins unchecked there, a 60 dB tilt most of them"""
    for name in R.ROUNDING:
        c = R.CASES[name]
        if c["features"]:
            share = R.unchecked_share(name)
            print("%s: %.4f %% unchecked" % (name, 100 * share))
            assert share <= c["unchecked_max"] and c["unchecked_max"] == (0.0 if c["signal"] == "white" else 0.01)
    assert {R.CASES[n]["signal"] for n in R.ROUNDING if R.CASES[n]["features"]} == {"white", "tilt"}
    white, tilt = R.unchecked_share("round-1024x256-B3"), R.unchecked_share("round-1024x256-tilt")
    print("n_fft 1024: white %.4f %%, tilt %.2f %% unchecked" % (100 * white, 100 * tilt))
    assert 0 < white < 0.01 < tilt
    # the tilted feature case does hold low-power bins: the top bin's mean power is more than 50 dB below the strongest bin's
    X, _, _ = R._round_reference("round-32x8-tilt")
    P = (X[:, 0::2] ** 2 + X[:, 1::2] ** 2).mean(axis=0)
    assert 10 * np.log10(P[-1] / P.max()) < -50


@pytest.mark.parametrize("name", R.SILENCE)
def test_silence_holds_for_the_float32_twin(name):
    R.check_silence(R.make_twin(), name)


@pytest.mark.parametrize("order", ["numpy", "chain"])
@pytest.mark.parametrize("name", R.CENTER)
def test_centred_wrapper_holds_for_the_float32_twin(name, order):
    assert 0 < R.check_center(R.make_twin(order), name, tag=TAG + "-" + order) <= 1


# ------------------------------------------------------------------------------------------ the mutants are rejected
MUTANT_CASES = [
    ("frame_offset", R.check_impulse, "imp-1024x256-j-exact"), ("frame_offset", R.check_impulse, "imp-96x100-T1"),
    ("frame_offset", R.check_rounding, "round-96x32-B3"),
    ("pad_next_row", R.check_impulse, "imp-1024x256-j-minus"), ("pad_next_row", R.check_impulse, "imp-96x100-j-plus"),
    ("pad_next_row", R.check_rounding, "round-1024x256-B3"),
    ("symmetric_hann", R.check_impulse, "imp-1024x256-16000"), ("symmetric_hann", R.check_rounding, "round-512x100-B3"),
    ("imag_sign", R.check_impulse, "imp-96x32-j-exact"), ("imag_sign", R.check_rounding, "round-32x8-B3"),
    ("f32_trig", R.check_impulse, "imp-1024x256-16000"), ("f32_trig", R.check_impulse, "imp-32x8-16000"),
    ("f32_trig", R.check_rounding, "round-1024x256-B3"), ("f32_trig", R.check_rounding, "round-32x8-B3"),
    ("f32_trig", R.check_rounding, "round-96x32-B3"), ("f32_trig", R.check_features, "round-32x8-feat"),
    ("bf16_operands", R.check_rounding, "round-1024x256-B3"), ("bf16_operands", R.check_rounding, "round-32x8-B3"),
    ("bf16_operands", R.check_features, "round-512x100-feat"),
    ("pad_columns", R.check_rounding, "round-96x32-B3"), ("pad_columns", R.check_rounding, "round-1024x256-43h"),
    ("no_eps", R.check_silence, "silence-1024x256"), ("no_eps", R.check_impulse, "imp-512x100-j-exact"),
    ("no_norm_eps", R.check_features, "round-32x8-feat"), ("no_norm_eps", R.check_silence, "silence-96x32"),
    ("legacy_transposed", R.check_impulse, "imp-256x64-16000"), ("legacy_transposed", R.check_rounding, "round-1024x256-tilt"),
    ("legacy_transposed", R.check_center, "center-256x64"),
]


def test_every_mutant_is_listed():
    assert {m for m, _, _ in MUTANT_CASES} == set(R.MUTANTS)


@pytest.mark.parametrize("mutant,check,name", MUTANT_CASES, ids=["%s-%s-%s" % (m, f.__name__, n) for m, f, n in MUTANT_CASES])
def test_mutant_is_rejected(mutant, check, name):
    kw = {} if check is R.check_silence else dict(tag=None)
    check(R.make_twin("numpy"), name, **kw)                   # the same evaluation passes without the mutation
    with pytest.raises(AssertionError):
        check(R.make_twin("numpy", mutant), name, **kw)


def _mutant_spectrum(name, mutant):
    c = R.CASES[name]
    X, E, chain = R._round_reference(name)
    got = R.twin_spectrum(R.signal(name), c["n_fft"], c["hop"], R.case_T(c), mutant=mutant)
    return R.element_ratio(got, X, E), R.rel_fro(got, X) / R.rel_fro(chain, X), got, E


@pytest.mark.parametrize("name", ["round-1024x256-B3", "round-96x32-B3", "round-32x8-B3"])
def test_the_element_bound_alone_passes_a_float32_basis(name):
    """why the aggregate is there: a basis whose cos, sin and Hann are evaluated in float32 with an unreduced phase stays
    inside the worst-case bound on every element that has one, and is many times the sequential twin in the relative
    Frobenius error.  (Of the element tier only the exact zeros notice it: Nyquist's sin column is sin(pi k) in float32.)"""
    worst, ratio, got, E = _mutant_spectrum(name, "f32_trig")
    print("%s float32-trig basis: worst error / bound %.3f, %.1f x the twin's relative Frobenius error" % (name, worst, ratio))
    assert worst <= 1 and ratio > 8
    assert (got[E == 0] != 0).any()


def test_bf16_operands_are_far_above_the_twin():
    """operands rounded to bf16: more than 1000 x the twin in the aggregate at every n_fft; the element bound is missed by
    several times at n_fft 1024"""
    for name in ("round-1024x256-B3", "round-256x64-B3", "round-32x8-B3"):
        worst, ratio, _, _ = _mutant_spectrum(name, "bf16_operands")
        print("%s bf16 operands: %.1f x the bound, %.0f x the twin's relative Frobenius error" % (name, worst, ratio))
        assert ratio > 1000 and (worst > 2 or name != "round-1024x256-B3")
