"""CPU tests of the STOI / ESTOI training loss (avvad_stoi_loss, csrc/stoi.hip): the float64 autograd reference of
tests/stoi_loss_ref.py against a central finite difference of the float64 score (so that a mistake is not restated), the
header's closed forms against autograd on one segment block, the hand-written chain against autograd, the float32 stand-in
against the float64 gradient -- which is where the GPU bound comes from -- the mutants, each of which the bound must
reject, and the host-side pieces that need no GPU (symbols, workspace query, refusals, the trainer's objective names)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import stoi_loss_ref as G
import stoi_ref as R
from conftest import ROOT

WITH_SEGMENT = [n for n in R.CASE_NAMES if G.has_segment(n)]


def test_reference_scores_are_stoi_refs():
    for name in R.CASE_NAMES:
        ref = R.reference(name)
        for which, key in ((1, "stoi"), (2, "estoi")):
            d, g = G.reference(name, which)
            assert abs(d - ref[key]) <= 1e-13, (name, key)
            assert g.shape == R.case(name)[1].shape
            if ref["segments"] == 0:
                assert d == 1e-5 and not g.any()


@pytest.mark.parametrize("name", WITH_SEGMENT)
def test_autograd_gradient_against_central_differences(name):
    """Three random directions per case and score.  The step moves every sample by about 1e-6 of the signal's rms: far
    below the smallest clip gap of the compared cases (1e-4), so no decision flips, and the truncation error (second order
    in 1e-6) is nothing.  What remains is the rounding of the two scores, about 2^-52 |d| each, over the difference 2 h |g.v|;
    the tolerance allows 64 of those roundings (the score is a sum over thousands of terms) plus 1e-7 relative."""
    fs, x, y = R.case(name)
    y64 = y.astype(np.float64)
    rng = np.random.default_rng(len(name) + y.size)
    for which in (1, 2):
        if which == 1 and name not in G.grad_cases(1):
            continue
        d, g = G.reference(name, which)
        for i in range(3):
            v = rng.standard_normal(y.size)
            h = 1e-6 * np.sqrt(np.mean(y64 ** 2))
            fd = -(G.score_of(x, y64 + h * v, fs, which) - G.score_of(x, y64 - h * v, fs, which)) / (2 * h)
            an = float(g @ v)
            tol = 1e-7 * abs(an) + 64 * 2.0 ** -52 * abs(d) / (2 * h)
            print("%-22s which %d direction %d: autograd %.9e central %.9e |diff| %.2e (tol %.2e)" % (name, which, i, an, fd, abs(an - fd), tol))
            assert abs(an - fd) <= tol


def test_closed_forms_against_autograd_on_one_block():
    rng = np.random.default_rng(5)
    X = rng.uniform(0.5, 2.0, (15, 30))
    Y = X * rng.uniform(0.6, 1.4, (15, 30))
    X[3, 7] = X[9, 20] = X[14, 0] = 0.5
    Y[3, 7], Y[9, 20], Y[14, 0] = 40.0, 55.0, 30.0             # a row's one large element: a y is about |x| = 7, above C x = 3.3
    gap, clipped, total = G.clip_stats(X, Y)
    assert clipped >= 3 and total == 450 and gap > 1e-3
    for which, closed in ((1, G.stoi_block_grad), (2, G.estoi_block_grad)):
        Yt = torch.tensor(Y, requires_grad=True)
        (-G.score_torch(X, Yt, which)).backward()
        want = Yt.grad.numpy()
        got = closed(X[None], Y[None])[0]
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), which
    # the clipped elements carry no direct gradient: with alpha held fixed their entries are exactly zero
    dy = G.stoi_block_grad(X[None], Y[None], alpha_const=True)[0]
    assert dy[3, 7] == dy[9, 20] == dy[14, 0] == 0.0 and np.count_nonzero(dy) == 450 - clipped


@pytest.mark.parametrize("name", ["k10_4097_one_segment", "k10_9001_half", "k16_11999", "k16_16000_half"])
def test_hand_written_chain_is_the_autograd_gradient(name):
    fs, x, y = R.case(name)
    for which in (1, 2):
        assert G.err(G.manual_grad(x, y, fs, which), G.reference(name, which)[1]) <= 1e-12


def test_the_gradient_cases_meet_their_conditions():
    stoi_cases, estoi_cases = G.grad_cases(1), G.grad_cases(2)
    assert estoi_cases == WITH_SEGMENT and "committed" in estoi_cases
    for name in estoi_cases:
        assert R.case_margin(name) >= R.MIN_MARGIN_DB
    for name in stoi_cases:
        assert G.case_clip(name)[0] >= G.MIN_CLIP_GAP
    assert "committed" not in stoi_cases and G.case_clip("committed")[0] < G.MIN_CLIP_GAP
    assert set(stoi_cases) == set(WITH_SEGMENT) - {"committed"}
    assert any(G.case_clip(n)[1] > 0 for n in stoi_cases) and any(G.case_clip(n)[1] == 0 for n in stoi_cases)
    assert G.case_clip("k10_4097_one_segment")[1] == 0 and G.case_clip("k16_10757")[1:] == (371, 9000)


def test_standin_is_within_an_eighth_of_the_gpu_bound():
    """where the bound comes from: MEASURED_STANDIN_GRAD is this test's worst figure, rounded up"""
    worst = 0.0
    for which in (1, 2):
        for name in G.grad_cases(which):
            fs, x, y = R.case(name)
            e = G.err(G.manual_grad(x, y, fs, which, f32=True), G.reference(name, which)[1])
            print("%-22s %s gradient: stand-in error %.3g" % (name, "STOI" if which == 1 else "ESTOI", e))
            worst = max(worst, e)
    print("worst %.4g, bound of the stand-in %.3g, GPU bound %.3g" % (worst, G.GPU_GRAD_BOUND / 8, G.GPU_GRAD_BOUND))
    assert G.GPU_GRAD_BOUND == 8 * G.MEASURED_STANDIN_GRAD
    assert 0.5 * G.MEASURED_STANDIN_GRAD <= worst <= G.GPU_GRAD_BOUND / 8


def test_chain_standin_is_within_an_eighth_of_its_gpu_bound():
    """the same derivation for dlogits of logits -> resynthesis -> loss"""
    worst = 0.0
    for which in (1, 2):
        c = G.chain_case(which)
        assert min(c["margin"]) >= R.MIN_MARGIN_DB and min(gap for gap, _, _ in c["clip"]) >= G.MIN_CLIP_GAP
        assert all(d > 0.5 for d in c["d64"])
        e = G.chain_err(c["y32"], c)
        print("chain %s: stand-in error %.3g" % ("STOI" if which == 1 else "ESTOI", e))
        worst = max(worst, e)
    print("worst %.4g, bound of the stand-in %.3g, GPU bound %.3g" % (worst, G.GPU_CHAIN_BOUND / 8, G.GPU_CHAIN_BOUND))
    assert G.GPU_CHAIN_BOUND == 8 * G.MEASURED_STANDIN_CHAIN
    assert 0.5 * G.MEASURED_STANDIN_CHAIN <= worst <= G.GPU_CHAIN_BOUND / 8


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_the_bound_rejects_every_mutant(mutant):
    moved = 0.0
    for name in ("k10_9001_half", "k16_16000_half", "k16_11999"):
        fs, x, y = R.case(name)
        for which in (1, 2):
            moved = max(moved, G.err(G.manual_grad(x, y, fs, which, mutant=mutant), G.reference(name, which)[1]))
    print("%s moves a gradient by %.3g (GPU bound %.3g)" % (mutant, moved, G.GPU_GRAD_BOUND))
    assert moved > 10 * G.GPU_GRAD_BOUND


def test_symbols_are_declared_bound_and_exported():
    from avvad import _lib as L
    h = L.lib()
    header = open(os.path.join(ROOT, "include", "avvad.h")).read()
    assert int(re.search(r"#define AVVAD_ABI_VERSION (\d+)", header).group(1)) == L.ABI_VERSION == h.avvad_abi_version() == 3
    for name in ("avvad_stoi_loss_workspace", "avvad_stoi_loss"):
        assert re.search(r"\b%s\(" % name, header) and name in L.SIGNATURES and getattr(h, name)
    assert len(L.SIGNATURES["avvad_stoi_loss_workspace"][1]) == 3 and len(L.SIGNATURES["avvad_stoi_loss"][1]) == 18
    assert len(L.SIGNATURES["avvad_stoi"][1]) == 15


def test_workspace_query_and_refusals_need_no_gpu():
    from avvad import _lib as L, ops
    h = L.lib()
    q = h.avvad_stoi_loss_workspace
    assert q(0, 100, 16000) == q(1, 0, 16000) == q(1, 100, 8000) == q(32768, 100, 10000) == 0
    small, big = q(1, 4096, 10000), q(1, 4097, 10000)
    assert 0 < small < big and small % 256 == 0 and big % 256 == 0        # 4097 samples: the first length with a segment
    for args in ((1, 4096, 10000), (1, 4097, 10000), (2, 48100, 16000), (16, 80000, 16000)):
        assert q(*args) > h.avvad_stoi_workspace(*args) > 0
    p = lambda v: C.c_void_p(v)                              # noqa: E731  (never dereferenced: every call is refused first)
    ok = [p(4096), 5000, p(8192), 5000, None, p(16384), 1, 5000, 16000, 1, p(32768), p(65536), p(131072), p(1 << 19), 5000,
          p(1 << 20), 1 << 30, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return h.avvad_stoi_loss(*a)
    assert call(a0=None) == call(a2=None) == call(a10=None) == call(a13=None) == call(a15=None) == -1
    assert call(a5=None) == -1                               # 16 kHz needs the taps
    assert call(a1=4999) == call(a3=4999) == call(a14=4999) == -1          # a pitch below L
    assert call(a8=8000) == call(a9=0) == call(a9=3) == call(a6=0) == call(a7=0) == -1
    assert call(a11=p(65540)) == call(a5=p(16388)) == call(a15=p((1 << 20) + 4)) == call(a12=p(131074)) == -1
    assert call(a16=q(1, 5000, 16000) - 4) == call(a11=None, a12=None, a16=q(1, 5000, 16000) - 4) == -2
    y = torch.zeros(5000)
    with pytest.raises(L.AvvadError, match="fs must be"):
        ops.stoi_loss(y, y, fs=8000)
    with pytest.raises(L.AvvadError, match="one shape"):
        ops.stoi_loss(y, torch.zeros(4999))
    with pytest.raises(L.AvvadError, match="no gradient"):
        ops.stoi_loss(y, torch.zeros(5000, requires_grad=True))
    with pytest.raises(L.AvvadError, match="GPU"):
        ops.stoi_loss(y, y)


def test_check_objective_takes_the_two_new_names():
    from avvad import train as TR
    assert TR.OBJECTIVES[:2] == ("bce", "si_sdr") and {"stoi", "estoi"} <= set(TR.OBJECTIVES)
    for name in ("stoi", "estoi"):
        TR.check_objective(name, "audio", False, [("a", "b")], 513)
        TR.check_objective(name, "audio", False, None, None, clean_wavs=["a"])
        for bad in (dict(kind="video"), dict(waveform=True), dict(wav_pairs=None), dict(y_dim=1)):
            kw = dict(kind="audio", waveform=False, wav_pairs=[("a", "b")], y_dim=513)
            kw.update(bad)
            with pytest.raises(ValueError, match=name):
                TR.check_objective(name, **kw)
    with pytest.raises(ValueError, match="one of"):
        TR.check_objective("pesq", "audio", False, [("a", "b")], 513)
    assert TR.StoiObjective("estoi", "cpu", None, lambda: None).extended and not TR.StoiObjective("stoi", "cpu", None, lambda: None).extended
