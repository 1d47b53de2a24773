"""The SI-SDR training path, the part that needs no GPU: the closed forms of tests/sisdr_ref.py (the adjoint of the masked
inverse STFT, the two-coefficient gradient of the loss) against float64 autograd, the mutants the assertion functions of
the GPU tests have to reject, the declared / bound / exported symbols and the trainer's argument checks."""
import os
import re

import numpy as np
import pytest

import sisdr_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("avvad_istft_bwd_workspace", "avvad_istft_bwd", "avvad_resynth_bwd_workspace", "avvad_resynth_bwd",
       "avvad_si_sdr_loss_workspace", "avvad_si_sdr_loss")


def _cases():
    """ragged, a hop that does not divide, centred and not, both modes; one with lengths below the natural ones and a scale"""
    return [S.cached_istft_case(64, 16, (9, 4, 1), 1, True, 1), S.cached_istft_case(64, 48, (5, 3), 2, True, 2),
            S.cached_istft_case(96, 24, (7, 2), 2, False, 3), _cut_case()]


def _cut_case():
    return S.cached_istft_case(64, 16, (9, 4, 1), 2, True, 4, lengths=(120, 70, 30), scale=(0.5, 2.0, 3.0))


def _loss_case():
    return S.sisdr_case([700, 300, 40, 0], 720, 24, 36, seed=5)


def test_closed_forms_equal_float64_autograd():
    for case in _cases():
        got, ref = S.dmask_closed(case), case["ref"]
        err = np.abs(got - ref).max()
        print("adjoint %d/%d mode %d: max|closed - autograd| = %.2e of %.2e" % (case["n_fft"], case["hop"], case["mode"], err, np.abs(ref).max()))
        assert err <= 1e-12 * np.abs(ref).max()
        S.check_dmask(S.dmask_closed, case)
    case = _loss_case()
    loss, ratios, grad, _, _ = S.sisdr_closed(case["est"], case["ref"], case["lengths"], case["head"], case["tail"])
    loss64, ratios64, grad64 = case["ref64"]
    err = np.abs(grad - grad64).max()
    print("loss: max|closed - autograd| = %.2e of %.2e" % (err, np.abs(grad64).max()))
    assert err <= 1e-12 * np.abs(grad64).max() and abs(loss - loss64) <= 1e-12 * abs(loss64)
    S.check_sisdr(lambda c: S.sisdr_closed(c["est"], c["ref"], c["lengths"], c["head"], c["tail"])[:3], case)
    # the float32 evaluation passes the same assertion
    S.check_sisdr(lambda c: S.sisdr_closed(c["est"], c["ref"], c["lengths"], c["head"], c["tail"], dtype=np.float32)[:3], case)


@pytest.mark.parametrize("name", sorted(S.MUTANTS))
def test_adjoint_mutants_are_rejected(name):
    case = _cut_case()
    S.check_dmask(S.dmask_closed, case)
    with pytest.raises(AssertionError):
        S.check_dmask(lambda c: S.dmask_closed(c, form=S.MUTANTS[name]), case, name=name)


@pytest.mark.parametrize("name", sorted(S.LOSS_MUTANTS))
def test_loss_mutants_are_rejected(name):
    case = _loss_case()
    with pytest.raises(AssertionError):
        S.check_sisdr(lambda c: S.sisdr_closed(c["est"], c["ref"], c["lengths"], c["head"], c["tail"], form=S.LOSS_MUTANTS[name])[:3],
                      case, name=name)


def test_new_symbols_are_declared_bound_and_exported():
    import ctypes
    from avvad import _lib as L
    header = open(os.path.join(ROOT, "include", "avvad.h")).read()
    declared = set(re.findall(r"\b(avvad_[a-z0-9_]+)\s*\(", header))
    h = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(h, name), name
    assert L.ABI_VERSION == 3 and int(re.search(r"#define AVVAD_ABI_VERSION (\d+)", header).group(1)) == 3
    h.avvad_abi_version.restype = ctypes.c_int
    assert h.avvad_abi_version() == 3


def test_objective_and_y_dim_are_validated():
    from avvad import train as TR
    pairs = [("noisy.wav", "clean.wav")]
    TR.check_objective("bce", "audio", False, None)
    TR.check_objective("si_sdr", "audio", False, pairs, 513)
    for args in (("mse", "audio", False, pairs), ("si_sdr", "audio", False, None), ("si_sdr", "audio", True, pairs),
                 ("si_sdr", "video", False, pairs), ("si_sdr", "audio", False, pairs, 1)):
        with pytest.raises(ValueError):
            TR.check_objective(*args)
    # train_main refuses before it touches a device
    with pytest.raises(ValueError):
        TR.train_main("audio", lambda: None, "x", wav_pairs=pairs, objective="mse")
    with pytest.raises(ValueError):
        TR.train_main("audio", lambda: None, "x", objective="si_sdr")
