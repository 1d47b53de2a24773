"""CPU tests of the noise-aware masks: the C ABI's new symbols and host-side tables, the float64 restatement
(tests/noise_aware_ref.py) against the reference's own masks (tests/golden/noise_aware.npz) outside a rounding band, the
mutants that comparison must reject, and the validation of ``mix_labels``."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import noise_aware_ref as R
from conftest import GOLDEN, ROOT, load_golden
from test_targets_cpu import IBM_DELTA

NAMES = ("avvad_target_noise_aware_workspace", "avvad_target_noise_aware_from_spectrum", "avvad_target_noise_aware")
LOW_CUT, HIGH_CUT = 5, 500
BAND_CAP = 0.01        # at most 1 % of the cells between the cuts may lie in a band


def sa1_pair():
    """(clean, noise) of the sa1 pair over the noisy file's peak, float32: what the fixture's spectra were made from"""
    clean = np.load("%s/utt_sa1_clean.npz" % GOLDEN)["samples"].astype(np.float32) / 32768.0
    noisy = np.load("%s/utt_sa1.npz" % GOLDEN)["samples"].astype(np.float32) / 32768.0
    peak = np.max(np.abs(noisy))
    return clean / peak, (noisy - clean) / peak


def golden_masks():
    g = load_golden("noise_aware")
    shape = tuple(int(v) for v in g["shape"])
    n = shape[0] * shape[1]
    return {k: np.unpackbits(g[k])[:n].reshape(shape).astype(bool) for k in ("speech", "noise", "threshold")}, g


@functools.lru_cache(maxsize=1)
def sa1_case():
    """float64 spectra of the pair, the tables, the reference's masks and the bands: computed once, never changed"""
    from avvad import ops
    s, n = sa1_pair()
    X, N = R.dft64(s), R.dft64(n)
    cs, cn = ops.noise_aware_tables(513)
    masks, _ = golden_masks()
    band_s, band_n = R.bands(X, N, cs, cn, IBM_DELTA)
    band_t, _ = R.bands(X, None, cs, cn, IBM_DELTA)
    inside = np.zeros(513, bool)
    inside[LOW_CUT - 1:HIGH_CUT] = True
    return dict(X=X, N=N, cs=cs, cn=cn, masks=masks, band=dict(speech=band_s, noise=band_n, threshold=band_t), inside=inside)


def banded_mismatches(ours, ref, band):
    """cells outside the band where the two masks differ"""
    return int(np.count_nonzero((ours != ref) & ~band))


def test_symbols_are_declared_bound_and_exported():
    from avvad import _lib as L
    h = L.lib()
    assert h.avvad_abi_version() == L.ABI_VERSION == 3
    header = open(os.path.join(ROOT, "include", "avvad.h")).read()
    declared = set(re.findall(r"\b(avvad_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in L.SIGNATURES and hasattr(h, name), name
    assert re.search(r"#define AVVAD_ABI_VERSION 3\b", header)


def test_tables_equal_the_reference_characteristic():
    from avvad import ops
    _, g = golden_masks()
    voiced, unvoiced = g["voiced"], g["unvoiced"]
    assert voiced.shape == unvoiced.shape == (513,) and voiced.dtype == np.float64
    cs, cn = ops.noise_aware_tables(513)
    assert cs.dtype == cn.dtype == np.float64
    np.testing.assert_allclose(cs, 10 ** ((0 * voiced + 5 * unvoiced) / 10), rtol=1e-15, atol=0)
    np.testing.assert_allclose(cn, 10 ** ((-10 * voiced + -10 * unvoiced) / 10), rtol=1e-15, atol=0)
    cs2, cn2 = ops.noise_aware_tables(513, 7, 1, -12, -8)
    np.testing.assert_allclose(cs2, 10 ** ((1 * voiced + 7 * unvoiced) / 10), rtol=1e-15, atol=0)
    np.testing.assert_allclose(cn2, 10 ** ((-12 * voiced + -8 * unvoiced) / 10), rtol=1e-15, atol=0)   # (sic: target.py:177)
    v, u = ops.voiced_unvoiced_characteristic(600)
    assert np.array_equal(v[:513], voiced) and np.array_equal(u[:504], unvoiced[:504]) and not u[504:].any()
    with pytest.raises(ValueError):
        ops.noise_aware_tables(504)


def test_workspace_query_rejects_bad_descriptors():
    from avvad import _lib as L
    h = L.lib()

    def ws(B=2, Lp=48100, n_fft=1024, hop=256, T=185, center=0):
        return h.avvad_target_noise_aware_workspace(C.byref(L.TargetDesc(B, Lp, n_fft, hop, T, center, 1e-8, 1.0, 1.0)))
    ld = 1028
    assert ws() >= 4 * (1024 * ld + 2 * 2 * 185 * ld)            # the basis and two spectra
    assert ws(B=0) == 0 and ws(hop=0) == 0 and ws(T=0) == 0 and ws(T=186) == 0
    assert ws(center=1) == 0 and ws(n_fft=1000) == 0 and ws(n_fft=0) == 0
    assert h.avvad_target_noise_aware_workspace(None) == 0
    # the clean-speech labels' query keeps its values
    d = L.TargetDesc(2, 48100, 1024, 256, 185, 0, 1e-8, 1.0, 1.0)
    assert 0 < h.avvad_target_workspace(C.byref(d)) < ws()


@pytest.mark.parametrize("which", ["speech", "noise", "threshold"])
def test_restatement_matches_reference_outside_the_band(which):
    c = sa1_case()
    N = None if which == "threshold" else c["N"]
    speech, noise, _ = R.noise_aware(c["X"], N, c["cs"], c["cn"])
    ours = noise if which == "noise" else speech
    ref, band = c["masks"][which], c["band"][which]
    assert ours.shape == ref.shape == (185, 513)
    frac = band[:, c["inside"]].mean()
    print("%s: %.3f %% of the cells between the cuts lie in the band, %d cells differ in all" % (which, 100 * frac, (ours != ref).sum()))
    assert frac <= BAND_CAP
    assert banded_mismatches(ours, ref, band) == 0
    # the cuts themselves: exact, band or not
    assert not ours[:, ~c["inside"]].any() if which != "noise" else ours[:, ~c["inside"]].all()
    assert np.array_equal(ours[:, ~c["inside"]], ref[:, ~c["inside"]])


def _mutants():
    """name -> (X, N, cs, cn) -> (speech, noise): restatements with one mistake each"""
    inf = float("inf")

    def low_cut_off_by_one(X, N, cs, cn):
        return R.noise_aware(X, N, cs, cn, low_cut=LOW_CUT + 1)[:2]         # cuts f < low_cut

    def rows_swapped(X, N, cs, cn):
        return R.noise_aware(X, N, cn, cs)[:2]

    def no_floor(X, N, cs, cn):
        return R.noise_aware(X, N, cs, cn, floor=-inf)[:2]                  # xs > -inf always, xn < -inf never

    def noise_and(X, N, cs, cn):
        p = R.parts(X, N, cs, cn)
        return R.noise_aware(X, N, cs, cn)[0], ((p["xn"] < p["nP"]) & (p["xn"] < 0.005)) | p["cut"]

    def noise_from_speech(X, N, cs, cn):
        return R.noise_aware(X, X, cs, cn)[:2]
    return dict(low_cut_off_by_one=low_cut_off_by_one, rows_swapped=rows_swapped, no_floor=no_floor, noise_and=noise_and,
                noise_from_speech=noise_from_speech)


@pytest.mark.parametrize("name", sorted(_mutants()))
def test_banded_comparison_rejects_mutant(name):
    c = sa1_case()
    speech, noise = _mutants()[name](c["X"], c["N"], c["cs"], c["cn"])
    bad = banded_mismatches(speech, c["masks"]["speech"], c["band"]["speech"]) + \
        banded_mismatches(noise, c["masks"]["noise"], c["band"]["noise"])
    print("%s: %d cells outside the bands differ" % (name, bad))
    assert bad >= 1


def test_mix_labels_are_validated_before_any_setup():
    from avvad import train

    def no_model():
        raise AssertionError("the model must not be built")
    for kw in (dict(mix_labels="ratio", clean_wavs=["a.wav"], noise_wavs=["n.wav"]),      # unknown name
               dict(mix_labels="irm"),                                                   # no mixture is made
               dict(mix_labels="noise_aware", wav_pairs=[("a.wav", "b.wav")])):
        with pytest.raises(ValueError, match="mix_labels"):
            train.train_main("audio", no_model, "unused", **kw)
    with pytest.raises(ValueError, match="mix_labels"):
        train.check_mix_labels("irm", True, y_dim=1)
    train.check_mix_labels("irm", True, y_dim=513)
    train.check_mix_labels("clean", False, y_dim=1)
    for kw in (dict(labels="vad_labels", mix_labels="irm"), dict(labels="ibm_labels", mix_labels="noisy")):
        with pytest.raises(ValueError, match="mix_labels"):
            train.mix_step(None, None, bank=None, draw=None, **kw)
