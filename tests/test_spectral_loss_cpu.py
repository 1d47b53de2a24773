"""The mask-regression losses (csrc/spectral_loss.hip), the part that needs no GPU: the float64 restatement of
tests/spectral_loss_ref.py against the values recorded from the reference's own three functions, the float32 stand-in
within the recorded bounds and each built-in mistake rejected at them (the loop mutants of a finish that stops after one
trip: rejected at "chunks130" / "rows67", accepted on every smaller shape), the declared / bound / exported symbols with the
chunk constant and the workspace query, the refusals of the C ABI with never-dereferenced pointers, and the argument
checks of ``check_objective``, ``train_main`` and ``ops.spectral_loss``."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import spectral_loss_ref as R
from conftest import ROOT

NEW = ("avvad_spectral_loss_workspace", "avvad_spectral_loss")
NAMES = ("mse_mask", "mse_signal", "msa")
GOLDEN = os.path.join(ROOT, "tests", "golden", "spectral_loss.npz")
ORIGINAL = ("one", "small", "ragged", "boundary", "three", "clamped", "saturated", "batch5")   # the shapes of at most 16 rows and 3 chunks


def golden_case(tag, kind):
    """one recorded utterance as a pred_mode 1 case of one full row, and the reference's own value for ``kind``"""
    g = np.load(GOLDEN)
    x, s = torch.from_numpy(g[tag + "_x"]), torch.from_numpy(g[tag + "_s"])
    T, F = x.shape
    c = {"name": "golden_%s" % tag, "kind": kind, "pred_mode": 1, "B": 1, "T": T, "F": F, "lengths": None,
         "pred": torch.from_numpy(g[tag + "_y_hat"])[None], "target": torch.from_numpy(g[tag + "_y"])[None], "mix": x[None],
         "speech": s[None]}
    return c, float(g[tag + "_loss"][R.KINDS.index(kind)])


@pytest.mark.parametrize("tag, shape", [("a", (5, 9)), ("b", (3, 513))])
def test_restatement_equals_the_recorded_reference(tag, shape):
    g = np.load(GOLDEN)
    assert g[tag + "_x"].shape == g[tag + "_s"].shape == g[tag + "_y"].shape == g[tag + "_y_hat"].shape == shape
    assert g[tag + "_x"].dtype == np.complex64 and 0.0 <= g[tag + "_y"].min() and g[tag + "_y"].max() <= 1.0
    assert 0.0 < g[tag + "_y_hat"].min() and g[tag + "_y_hat"].max() < 1.0
    for kind in R.KINDS:
        c, want = golden_case(tag, kind)
        loss, rows, dpred = R.reference(c)
        assert abs(loss - want) <= 1e-12 * abs(want) and abs(rows[0] - want) <= 1e-12 * abs(want), (kind, loss, want)
        assert dpred.shape == (1,) + shape and np.isfinite(dpred).all()


def test_case_list_has_the_shapes_the_kernel_can_go_wrong_at():
    assert R.n_chunks(R.T3, 513) == 3 and R.T3 % 2 == 1
    B, T, F, lens = R.SHAPES["boundary"]
    assert F == 1 and sorted(lens) == [R.CHUNK - 1, R.CHUNK, R.CHUNK + 1] and T > max(lens) and R.n_chunks(T, F) == 2
    assert R.SHAPES["ragged"][:3] == (3, 7, 513) and R.SHAPES["ragged"][3] == (7, 4, 0)
    assert R.lens_of(R.case("clamped", "mask", 1)) == [3, 0]
    sat = R.case("saturated", "mask", 2)["pred"]
    assert {30.0, -30.0, 100.0, -100.0} <= set(sat[0].reshape(-1).tolist())
    assert len(R.CASES) == 3 * (2 * len(R.SHAPES) - 1)
    # the finishing loops: a wave adds a row's partials 64 at a time, 16 waves take a row each, 64 lanes add the rows
    B, T, F, lens = R.SHAPES["chunks130"]
    assert [R.n_chunks(n, F) for n in lens] == [130, 65, 64, 0] and R.n_chunks(T, F) == 130 and F % 2 == 1 and T % 2 == 1
    assert B == len(lens) == 4 and sum(n == 0 for n in lens) <= 1 and max(lens) == T
    B, T, F, lens = R.SHAPES["rows67"]
    assert B == len(lens) == 67 > 64 and -(-B // 16) == 5 and -(-B // 64) == 2 and max(lens) <= T
    assert lens[64:] == (5, 3, 7) and all(n > 0 for n in lens[64:]) and all(lens[b] > 0 for b in (16, 17, 32, 48, 63))
    assert set(ORIGINAL) | {"chunks130", "rows67"} == set(R.SHAPES) and len(ORIGINAL) == 8
    assert all(R.SHAPES[n][0] <= 16 and R.n_chunks(*R.SHAPES[n][1:3]) <= 64 for n in ORIGINAL)


@pytest.mark.parametrize("name, kind, pred_mode", R.CASES)
def test_float32_standin_stays_within_the_bounds(name, kind, pred_mode):
    c = R.case(name, kind, pred_mode)
    loss, rows, dpred = R.check_spectral(R.standin, c)
    for b, n in enumerate(R.lens_of(c)):
        assert (n == 0) == (rows[b] == 0.0)


def test_recorded_bounds_are_eight_times_the_standin():
    worst = R.measure_standin()
    for bound, w in zip((R.BOUND_LOSS, R.BOUND_ROWS, R.BOUND_DPRED), worst):
        assert bound / 16 <= w <= bound / 4, (bound, w)      # (a host's float32 sigmoid may differ in the last bit or two)


def test_a_row_alone_is_a_case_of_its_own():
    c = R.case("batch5", "spectrum", 2)
    whole = R.standin(c)
    for b in (1, 4):
        one = R.check_spectral(R.standin, R.single_row(c, b))
        assert one[1][0] == whole[1][b] and np.array_equal(one[2][0], whole[2][b])


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_each_mutant_is_rejected(mutant):
    kind, pred_mode = R.MUTANTS[mutant]
    c = R.case("ragged", kind, pred_mode)
    R.check_spectral(R.standin, c)
    with pytest.raises(AssertionError):
        R.check_spectral(lambda case: R.standin(case, mutant), c)


@pytest.mark.parametrize("mutant", sorted(R.LOOP_MUTANTS))
def test_each_loop_mutant_is_rejected_on_its_new_case_alone(mutant):
    """a finish that stops after one trip of one of its three loops: rejected by the shape that turns that loop, and
    accepted on every shape the list had before -- none of them could see it"""
    name, kind, pred_mode = R.LOOP_MUTANTS[mutant]
    broken = lambda case: R.standin(case, mutant)                                       # noqa: E731
    c = R.case(name, kind, pred_mode)
    R.check_spectral(R.standin, c)
    with pytest.raises(AssertionError):
        R.check_spectral(broken, c)
    for old in ORIGINAL:
        c = R.case(old, kind, pred_mode)
        got = R.check_spectral(broken, c)
        want = R.standin(c)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (mutant, old)


def test_spectral_symbols_are_declared_bound_and_exported():
    from avvad import _lib as L, ops
    h = L.lib()
    assert h.avvad_abi_version() == L.ABI_VERSION == 3            # added entry points change no signature
    header = open(os.path.join(ROOT, "include", "avvad.h")).read()
    assert int(re.search(r"#define AVVAD_ABI_VERSION (\d+)", header).group(1)) == 3
    declared = set(re.findall(r"\b(avvad_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(h, name), name
    build = open(os.path.join(ROOT, "audio-visual-vad_amd", "csrc", "build.sh")).read()
    assert re.search(r'SRCS="[^"]*\bspectral_loss\b[^"]*"', build)
    assert R.CHUNK == L.SPECTRAL_CHUNK == ops.SPECTRAL_CHUNK
    source = open(os.path.join(ROOT, "audio-visual-vad_amd", "csrc", "spectral_loss.hip")).read()
    assert re.search(r"constexpr int CHUNK = AVVAD_SPECTRAL_CHUNK;", source)
    assert ops.SPECTRAL_KINDS == {"mask": 0, "signal": 1, "spectrum": 2}


def test_workspace_query():
    from avvad import _lib as L
    h = L.lib()
    chunk = L.SPECTRAL_CHUNK
    # one double per (row, chunk) rounded up to 256 bytes, then one double per row rounded up likewise
    assert h.avvad_spectral_loss_workspace(1, 1, 1) == h.avvad_spectral_loss_workspace(1, 32, chunk) == 512
    assert h.avvad_spectral_loss_workspace(1, 32 * chunk + 1, 1) == 512 + 256
    assert h.avvad_spectral_loss_workspace(16, 300, 513) == 16 * -(-300 * 513 // chunk) * 8 + 256
    assert h.avvad_spectral_loss_workspace(33, 1, chunk) == 512 + 512
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (65536, 1, 1), (1, 1 << 16, (1 << 14) + 1), (-1, 3, 3)):
        assert h.avvad_spectral_loss_workspace(*bad) == 0, bad
    assert h.avvad_spectral_loss_workspace(1, 1 << 16, 1 << 14) > 0


def test_refusals_need_no_gpu():
    from avvad import _lib as L
    h = L.lib()
    p = lambda v: C.c_void_p(v)                              # noqa: E731  (never dereferenced: every call is refused first)
    B, T, F = 2, 3, 5
    #      pred   mode kind target     mix        mb         mt     mf speech     sb         st     sf
    ok = [p(0x1000), 2, 2, p(0x2000), p(0x3000), 2 * T * F, 2 * F, 2, p(0x4000), 2 * T * F, 2 * F, 2,
          # n_frames loss      row_loss   dpred      B  T  F  ws          bytes stream
          p(0x5000), p(0x6000), p(0x7000), p(0x8000), B, T, F, p(0x10000), 512, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return h.avvad_spectral_loss(*a)
    for i in (0, 4, 8, 13, 19):                              # a NULL where kind 2 needs a pointer
        assert call(**{"a%d" % i: None}) == -1, i
    assert call(a2=1, a3=None) == call(a2=0, a3=None) == call(a2=1, a4=None) == -1      # kind 0 / 1: target, kind 1: mix
    assert call(a2=-1) == call(a2=3) == call(a1=0) == call(a1=3) == -1                  # unknown kind / pred_mode
    assert call(a16=0) == call(a16=65536) == call(a17=0) == call(a18=0) == call(a17=1 << 16, a18=(1 << 14) + 1) == -1
    assert call(a5=3) == call(a6=0) == call(a7=1) == call(a10=-2) == call(a5=0) == call(a9=-2) == -1   # odd / non-positive strides
    assert call(a4=p(0x3004)) == call(a8=p(0x4004)) == call(a14=p(0x7004)) == -1        # spectra / row_loss off their 8 bytes
    assert call(a19=p(0x10004)) == call(a19=p(0x10008)) == -1                           # ws off its 16 bytes
    assert call(a20=511) == -2                                                          # one byte short
    assert call(a2=0, a4=None, a8=None, a20=511) == -2       # (kind 0 reads no spectrum: its pointers do not count)
    assert call(a12=None, a14=None, a15=None, a20=511) == -2  # (the optional ones)


def test_ops_refuses_cpu_tensors_wrong_dtypes_and_shapes():
    from avvad import _lib as L, ops
    pred, y = torch.zeros(2, 3, 5), torch.zeros(2, 3, 5)
    with pytest.raises(L.AvvadError, match="GPU"):
        ops.spectral_loss(pred, "mask", target=y)
    with pytest.raises(L.AvvadError, match="kind"):
        ops.spectral_loss(pred, "mse", target=y)
    with pytest.raises(L.AvvadError, match="pred_mode"):
        ops.spectral_loss(pred, "mask", target=y, pred_mode=0)
    from packages.models import utils as U
    for name in ("mean_square_error_mask", "mean_square_error_signal", "magnitude_spectrum_approxiamation_loss"):
        assert callable(getattr(U, name))
    with pytest.raises(L.AvvadError, match="GPU"):
        U.mean_square_error_mask(y[0], pred[0])
    assert "not provided" not in U.__doc__.split("VAE")[0]


def test_objectives_are_accepted_under_the_conditions_of_si_sdr():
    from avvad import train as TR
    pairs = [("noisy.wav", "clean.wav")]
    assert set(NAMES) <= set(TR.OBJECTIVES) and "mse" not in TR.OBJECTIVES
    assert {TR.SPECTRAL_OBJECTIVES[n] for n in NAMES} == set(R.KINDS)
    for name in NAMES:
        TR.check_objective(name, "audio", False, pairs)
        TR.check_objective(name, "audio", False, pairs, 513)
        TR.check_objective(name, "audio", False, None, 513, clean_wavs=["a.wav"])
        for args, kw in (((name, "video", False, pairs), {}), ((name, "AV", False, pairs), {}), ((name, "audio", True, pairs), {}),
                         ((name, "audio", False, pairs, 1), {}), ((name, "audio", False, None, 513), {}),
                         ((name, "audio", False, None, 1), {"clean_wavs": ["a.wav"]})):
            with pytest.raises(ValueError, match=name):
                TR.check_objective(*args, **kw)


def test_train_main_refuses_before_touching_a_device(tmp_path, monkeypatch):
    from avvad import train as TR
    never = lambda: pytest.fail("the model must not be built before the arguments are checked")   # noqa: E731
    kw = dict(out_dir=str(tmp_path))
    for name in NAMES:
        with pytest.raises(ValueError, match=name):
            TR.train_main("audio", never, "m", objective=name, **kw)                    # no data source
        with pytest.raises(ValueError, match=name):
            TR.train_main("video", never, "m", objective=name, wav_pairs=[("a", "b")], **kw)
        with pytest.raises(ValueError, match=name):
            TR.train_main("audio", never, "m", waveform=True, objective=name, wav_pairs=[("a", "b")], **kw)
    monkeypatch.setenv("AVVAD_OBJECTIVE", "msa")             # the override names the new objectives too
    with pytest.raises(ValueError, match="msa"):
        TR.train_main("audio", never, "m", **kw)
