"""GPU tests of the STOI / ESTOI training loss (csrc/stoi.hip avvad_stoi_loss, ops.stoi_loss, train.StoiObjective) against
the float64 autograd reference tests/stoi_loss_ref.py on stoi_ref's shared inputs.

The score must be ``ops.stoi``'s bit for bit and within stoi_ref.GPU_BOUND of float64.  The gradient's error per row,
max|g - g64| / max|g64|, must lie within stoi_loss_ref.GPU_GRAD_BOUND = 8 x the float32 stand-in's worst figure (2.32e-5);
the ESTOI gradient wherever there is a segment, the STOI gradient where the reference's clip gap allows it (every case but
the committed utterance).  These cases stop at 233 frames and 5 rows; tests/test_stoi_long_gpu.py carries the same checks
past 256 and 1024 frames and past 64 rows.  Then the contracts: a row alone = its bits in a ragged batch, also under a CU
cap, zeros behind every length, run to run, pitches, the upstream scale, the refusal, the chain from the logits (GPU_CHAIN_BOUND, 6.16e-6)
and a training run."""
import ctypes as Ct
import os
import re

import numpy as np
import pytest
import torch

import stoi_loss_ref as G
import stoi_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_ = torch.tensor
NAN = float("nan")

CASES = ["k10_4097_one_segment", "k10_4096_no_segment", "k10_9001_half", "k16_16000_half", "k16_8192", "k16_8705", "k16_9218",
         "k16_9731", "k16_10244", "k16_10757", "k16_11270", "k16_11999", "committed"]


def _ops():
    from avvad import ops
    return ops


_ALONE = {}


def _alone(name, which):
    """(loss (), d (1,), gradient (L,)) of a case on its own, computed once"""
    if (name, which) not in _ALONE:
        fs, x, y = R.case(name)
        yd = T_(y).to(DEV).requires_grad_(True)
        loss, d = _ops().stoi_loss(yd, T_(x).to(DEV), fs=fs, extended=which == 2, return_scores=True)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and d.dtype == torch.float64 and d.shape == (1,) and not d.requires_grad
        loss.backward()
        _ALONE[(name, which)] = (loss.detach(), d, yd.grad.clone())
    return _ALONE[(name, which)]


def test_the_compared_cases_cover_both_clip_branches():
    compared = [n for n in CASES if n in G.grad_cases(1)]
    assert any(G.case_clip(n)[1] > 0 for n in compared) and any(G.case_clip(n)[1] == 0 for n in compared)
    assert len({R.case(n)[1].size % 8 for n in CASES if n.startswith("k16_") and R.case(n)[1].size < 12000}) == 8


@pytest.mark.parametrize("name", CASES)
def test_value_and_gradient_against_float64(name):
    ops = _ops()
    fs, x, y = R.case(name)
    ref = R.reference(name)
    assert R.case_margin(name) >= R.MIN_MARGIN_DB
    scored = ops.stoi(T_(x).to(DEV), T_(y).to(DEV), fs=fs, both=True)[0]
    for which, key in ((1, "stoi"), (2, "estoi")):
        loss, d, grad = _alone(name, which)
        d64, g64 = G.reference(name, which)
        g = grad.cpu().numpy()
        assert g.shape == g64.shape and np.isfinite(g).all()
        print("%-22s %-5s d %.9f |d - float64| = %.3g (bound %.3g)" % (name, key, float(d), abs(float(d) - d64), R.GPU_BOUND))
        assert torch.equal(d.view(torch.int64), scored[which - 1:which].view(torch.int64))
        assert abs(float(d) - ref[key]) <= R.GPU_BOUND
        assert float(loss) == float(np.float32(-float(d)))
        if ref["segments"] == 0:
            assert float(d) == 1e-5
        G.check_gradient(name, which, g)       # zeros without a segment, else the error where the gradient is compared


def _batch(names, P):
    """rows of pitch P holding the named cases (one rate), NaN behind each row's length; "short": 200 samples"""
    x = np.full((len(names), P), NAN, dtype=np.float32)
    y = x.copy()
    lengths = []
    for b, n in enumerate(names):
        if n == "short":
            x[b, :200], y[b, :200] = 0.1, 0.2
            lengths.append(200)
            continue
        _, cx, cy = R.case(n)
        x[b, :cx.size], y[b, :cx.size] = cx, cy
        lengths.append(cx.size)
    return T_(x).to(DEV), T_(y).to(DEV), lengths


@pytest.mark.parametrize("fs, names", [
    (10000, ["k10_9001_half", "k10_4097_one_segment", "short", "k10_4096_no_segment", "k10_6000_light"]),
    (16000, ["k16_16000_half", "k16_8705", "short", "k16_9731", "k16_11999"]),
])
def test_ragged_batch_rows_keep_their_bits(fs, names, lib_options):
    """B = 5 with a 200-sample row, NaN behind every length, a pitch wider than L: every row's gradient has the bits it has
    alone, at max_cus 0 and 24; exact zeros behind each length; the run repeats bit for bit"""
    ops = _ops()
    L = max(R.case(n)[1].size for n in names if n != "short")
    P = L + 37
    x, y, lengths = _batch(names, P)
    for which in (1, 2):
        runs = []
        for cap in (0, 24, 0):
            lib_options("max_cus", cap)
            wide = y.clone().requires_grad_(True)
            loss, d = ops.stoi_loss(wide[:, :L], x[:, :L], lengths=lengths, fs=fs, extended=which == 2, return_scores=True)
            loss.backward()
            g = wide.grad
            assert d.shape == (5,) and g.shape == (5, P) and bool(torch.isfinite(g).all())
            total = 0.0
            for b, n in enumerate(names):
                assert torch.count_nonzero(g[b, lengths[b]:]).item() == 0
                total += float(d[b])
                if n == "short":
                    assert float(d[b]) == 1e-5 and torch.count_nonzero(g[b]).item() == 0
                    continue
                _, da, ga = _alone(n, which)
                assert torch.equal(d[b:b + 1].view(torch.int64), da.view(torch.int64)), (n, cap)
                assert torch.equal(g[b, :lengths[b]], ga), (n, cap)
            assert float(loss.detach()) == float(np.float32(-total))
            runs.append((loss.detach(), g.clone()))
        assert torch.equal(runs[0][0], runs[2][0]) and torch.equal(runs[0][1], runs[2][1])


def test_pitched_gradient_through_the_c_abi():
    """dproc at a pitch 13 floats wider than L: columns 0 .. L - 1 are the op's bits, the rest is not touched; d and info
    may be NULL"""
    from avvad import _lib as L
    ops = _ops()
    lib = L.lib()
    names = ["k16_11999", "k16_9218"]
    n = max(R.case(k)[1].size for k in names)
    x, y, lengths = _batch(names, n + 5)
    lens = T_(lengths, dtype=torch.int32).to(DEV)
    taps = T_(ops.stoi_taps()).to(DEV)
    nbytes = lib.avvad_stoi_loss_workspace(2, n, 16000)
    stream = Ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    for which in (1, 2):
        ws = torch.empty(nbytes // 4, device=DEV)
        loss = torch.full((1,), NAN, device=DEV)
        dproc = torch.full((2, n + 13), NAN, device=DEV)
        rc = lib.avvad_stoi_loss(L.ptr(x), n + 5, L.ptr(y), n + 5, L.ptr(lens), L.ptr(taps), 2, n, 16000, which, L.ptr(loss), None, None,
                                 L.ptr(dproc), n + 13, L.ptr(ws), nbytes, stream)
        assert rc == 0
        assert bool(torch.isnan(dproc[:, n:]).all())
        total = 0.0
        for b, k in enumerate(names):
            _, da, ga = _alone(k, which)
            total += float(da)
            assert torch.equal(dproc[b, :lengths[b]], ga) and torch.count_nonzero(dproc[b, lengths[b]:n]).item() == 0
        assert float(loss) == float(np.float32(-total))


def test_upstream_scale_and_refusals():
    ops = _ops()
    fs, x, y = R.case("k16_9218")
    xd = T_(x).to(DEV)
    for which in (1, 2):
        yd = T_(y).to(DEV).requires_grad_(True)
        (ops.stoi_loss(yd, xd, fs=fs, extended=which == 2) * 0.5).backward()
        assert torch.equal(yd.grad, _alone("k16_9218", which)[2] * 0.5)
    with pytest.raises(ops.L.AvvadError, match="no gradient"):
        ops.stoi_loss(T_(y).to(DEV).requires_grad_(True), xd.clone().requires_grad_(True), fs=fs)
    with torch.no_grad():
        assert ops.stoi_loss(T_(y).to(DEV), xd, fs=fs).grad_fn is None
    yd = T_(y).to(DEV).requires_grad_(True)
    loss = ops.stoi_loss(yd, xd, fs=fs)
    (g,) = torch.autograd.grad(loss, yd, create_graph=True)
    with pytest.raises(RuntimeError):                           # no double backward
        g.sum().backward()


@pytest.mark.parametrize("which", [1, 2])
def test_chain_from_logits_to_their_gradient(which):
    """logits -> resynth -> stoi_loss -> dlogits at 1024 / 256, B = 2 ragged, the first and last n_fft - hop samples sliced
    off, against the float64 chain; the scores are ops.stoi's of the same estimate; two runs give the same bits"""
    ops = _ops()
    case = G.chain_case(which)
    assert min(case["margin"]) >= R.MIN_MARGIN_DB and min(gap for gap, _, _ in case["clip"]) >= G.MIN_CLIP_GAP
    noisy, clean = T_(case["noisy"]).to(DEV), T_(case["clean"]).to(DEV)
    skip, lens = case["skip"], case["lengths"]
    inner = [n - 2 * skip for n in lens]
    runs = []
    for _ in range(2):
        logits = T_(case["mask"]).to(DEV).requires_grad_(True)
        est = ops.resynth(noisy, logits, mask_mode=2, n_fft=case["n_fft"], hop=case["hop"], sample_lengths=lens)
        n = est.shape[1]
        assert max(lens) - case["hop"] <= n <= clean.shape[1]
        loss, d = ops.stoi_loss(est[:, skip:n], clean[:, skip:n], inner, fs=16000, extended=which == 2, return_scores=True)
        loss.backward()
        runs.append((loss.detach(), logits.grad.clone()))
    loss, grad = runs[0]
    assert torch.equal(loss, runs[1][0]) and torch.equal(grad, runs[1][1])
    scored = ops.stoi(clean[:, skip:n], est.detach()[:, skip:n], lengths=inner, fs=16000, extended=which == 2)
    assert torch.equal(scored.view(torch.int64), d.view(torch.int64))
    assert float(loss) == float(np.float32(-(float(d[0]) + float(d[1]))))
    g = grad.cpu().numpy()
    assert np.isfinite(g).all()
    for b, nf in enumerate(case["frames"]):
        assert not g[b, nf:].any()
    e = G.chain_err(g, case)
    print("chain which %d: loss %.7f float64 %.7f, d %s float64 %s, dlogits error %.3g (bound %.3g)"
          % (which, float(loss), case["loss64"], d.tolist(), case["d64"], e, G.GPU_CHAIN_BOUND))
    assert e <= G.GPU_CHAIN_BOUND


def test_training_on_estoi(tmp_path):
    """DeepVAD_audio (513 bins, one layer, hidden 32) on the committed noisy / clean pair, used twice as a batch: Adam at
    1e-3, 8 steps.  The step-8 loss is below the step-1 loss, two runs from the same seed end in the same parameter bits and
    the log line carries the batch's mean score (the loss is minus the sum of the two rows)."""
    from avvad import train as TR
    from packages.models.Audio_Net import DeepVAD_audio
    pair = (os.path.join(GOLDEN, "utt_sa1.npz"), os.path.join(GOLDEN, "utt_sa1_clean.npz"))
    states, losses = [], []
    for run in ("a", "b"):
        out = str(tmp_path / run)
        model = TR.train_main("audio", lambda: DeepVAD_audio(1, 32, 513), "estoi", epochs=8, batch_size=2, lr=1e-3, out_dir=out,
                              wav_pairs=[pair, pair], objective="estoi")
        states.append({k: v.detach().clone() for k, v in model.state_dict().items()})
        log = open(os.path.join(out, "output_batch.log")).read()
        steps = re.findall(r"train batch +0  loss (\S+) .* estoi (\S+)", log)
        assert len(steps) == 8, log
        assert all(abs(float(a) + 2 * float(b)) < 1e-3 for a, b in steps)            # loss = -(sum of two rows), printed to 3 digits
        losses.append([-2 * float(b) for _, b in steps])
    print("estoi: training loss per step", losses[0])
    assert losses[0][7] < losses[0][0], losses[0]
    assert losses[0] == losses[1]
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k
