"""Training on SI-SDR on the GPU: the gradient of ``ops.istft`` / ``ops.resynth`` with respect to the mask or its logits
(avvad_istft_bwd, avvad_resynth_bwd), ``ops.si_sdr_loss`` (avvad_si_sdr_loss), the whole chain and
``train_main(objective="si_sdr")``, against the float64 references of tests/sisdr_ref.py.

The bound of every float32 GEMM result is ``8 E_cpu32``: ``E_cpu32 = max |yardstick - float64|`` of the same chain evaluated
in float32 in the GEMM form on the CPU, on the same inputs (``istft_ref.FACTOR``, the margin the forward's tests grant).
Both go to the parity log.  Exact properties -- zeros in the padding frames and outside the loss window, the forward's
bits, the fused call against its halves, run-to-run bits -- are compared bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

import sisdr_ref as S
from conftest import GOLDEN
from test_gpu_parity import _report as _parity_report

pytestmark = pytest.mark.gpu
T_ = torch.from_numpy
DEV = "cuda:0"
PARITY = [(64, 16, (9, 4, 1)), (96, 24, (7, 2)), (64, 48, (5, 3)), (1024, 256, (130, 5))]


def _report(name, got, ref, atol):
    _parity_report("sisdr: " + name, got, ref, atol)


def _scale(case):
    return None if case["scale"] is None else T_(case["scale"]).to(DEV)


def _istft_grad(case, legacy=False):
    """dmask of ops.istft on the case's NaN-padded buffers"""
    from avvad import ops
    spec = T_(case["spec"]).to(DEV)
    if legacy:
        spec = spec[0].permute(1, 0, 2).contiguous()            # (F, T, 2) of ONE utterance
    m = T_(case["mask"]).to(DEV).requires_grad_(True)
    out = ops.istft(spec, case["n_fft"], case["hop"], mask=m, mask_mode=case["mode"], n_frames=case["frames"],
                    length=case["lengths"], center=case["center"], scale=_scale(case))
    assert out.grad_fn is not None
    out.backward(T_(case["dout"]).to(DEV))
    return m.grad.cpu().numpy()


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n_fft,hop,frames", PARITY)
def test_mask_gradient_of_istft(n_fft, hop, frames, mode, center):
    """dmask (mode 1) and dlogit (mode 2) on the forward's own ragged shapes: a one-frame row, a length that is no power of
    two, a hop that does not divide, 260 GEMM rows across the 128-row tiles.  center=True: a full random cotangent (the
    window sum of squares stays >= 0.043); center=False: zero in the first and last n_fft - hop samples.  The padding
    frames of spec and mask and dout behind each row's length hold NaN."""
    case = S.cached_istft_case(n_fft, hop, frames, mode, center, 100 + n_fft + hop)
    S.check_dmask(_istft_grad, case, _report, "istft %d/%d mode %d center %d" % (n_fft, hop, mode, center))


def test_lengths_below_the_natural_ones_and_a_scale():
    case = S.cached_istft_case(64, 16, (9, 4, 1), 2, True, 4, lengths=(120, 70, 30), scale=(0.5, 2.0, 3.0))
    S.check_dmask(_istft_grad, case, _report, "istft 64/16 cut lengths, scale")


def test_resynth_backward_equals_its_halves_and_the_reference():
    """ops.resynth's backward against ops.stft_complex -> ops.istft's backward bit for bit, and against float64 at
    1024 / 256 with ragged sample lengths and a non-unit scale; ops.istft on the legacy (F, T, 2) layout."""
    from avvad import ops
    n_fft, hop, lens = 1024, 256, [5000, 3300]
    rng = np.random.default_rng(11)
    wave = np.zeros((2, max(lens)), dtype=np.float32)
    for b, n in enumerate(lens):
        wave[b, :n] = rng.standard_normal(n) * 0.3
    wd = T_(wave).to(DEV)
    frames = [ops.n_frames(n, n_fft, hop) for n in lens]
    spec = ops.stft_complex(wd, n_fft, hop)
    assert spec.shape[1] == max(frames)
    for mode in (1, 2):
        case = S.istft_case(n_fft, hop, frames, mode, False, 12 + mode, lengths=lens, scale=(0.5, 1.75),
                            spec_rows=list(spec.cpu().numpy()))
        mask = np.nan_to_num(case["mask"], nan=0.25)            # (the halves must see the same padding to give the same bits)
        dout = T_(case["dout"]).to(DEV)
        grads, outs = [], []
        for fused in (True, False):
            m = T_(mask).to(DEV).requires_grad_(True)
            if fused:
                out = ops.resynth(wd, m, mask_mode=mode, n_fft=n_fft, hop=hop, sample_lengths=lens, scale=_scale(case))
            else:
                out = ops.istft(spec, n_fft, hop, mask=m, mask_mode=mode, n_frames=frames, length=lens, scale=_scale(case))
            out.backward(dout)
            grads.append(m.grad)
            outs.append(out.detach())
        assert torch.equal(outs[0], outs[1]) and torch.equal(grads[0], grads[1])
        S.check_dmask(lambda c: grads[0].cpu().numpy(), case, _report, "resynth 1024/256 mode %d ragged, scale" % mode)
    one = S.cached_istft_case(1024, 256, (6,), 2, True, 15)
    S.check_dmask(lambda c: _istft_grad(c, legacy=True), one, _report, "istft legacy (F,T,2) 1024/256")


def test_forward_bits_are_unchanged_and_modes_0_and_3_build_no_graph():
    from avvad import ops
    case = S.cached_istft_case(64, 16, (9, 4, 1), 2, True, 100 + 64 + 16)
    spec = T_(np.nan_to_num(case["spec"])).to(DEV)
    logits = T_(np.nan_to_num(case["mask"])).to(DEV)
    wave = torch.randn(2, 700, device=DEV) * 0.3
    wl = torch.randn(2, ops.n_frames(700, 64, 16), 33, device=DEV)
    for mode in (1, 2):
        m = logits.clone().requires_grad_(True)
        with_graph = ops.istft(spec, 64, 16, mask=m, mask_mode=mode, n_frames=case["frames"])
        with torch.no_grad():
            plain = ops.istft(spec, 64, 16, mask=m, mask_mode=mode, n_frames=case["frames"])
        assert with_graph.grad_fn is not None and plain.grad_fn is None and torch.equal(with_graph, plain)
        assert torch.equal(plain, ops.istft(spec, 64, 16, mask=logits, mask_mode=mode, n_frames=case["frames"]))
        w = wl.clone().requires_grad_(True)
        with_graph = ops.resynth(wave, w, mask_mode=mode, n_fft=64, hop=16, sample_lengths=[700, 431])
        with torch.no_grad():
            plain = ops.resynth(wave, w, mask_mode=mode, n_fft=64, hop=16, sample_lengths=[700, 431])
        assert with_graph.grad_fn is not None and plain.grad_fn is None and torch.equal(with_graph, plain)
    m = logits.clone().requires_grad_(True)
    assert ops.istft(spec, 64, 16, mask=m, mask_mode=3, n_frames=case["frames"]).grad_fn is None
    assert ops.istft(spec, 64, 16, n_frames=case["frames"]).grad_fn is None
    w = wl.clone().requires_grad_(True)
    assert ops.resynth(wave, w, mask_mode=3, n_fft=64, hop=16).grad_fn is None
    assert ops.resynth(wave, None, mask_mode=0, n_fft=64, hop=16).grad_fn is None


def _loss_impl(pad):
    """ops.si_sdr_loss on rows ``pad`` floats wider than L, read and differentiated in place"""
    def impl(case):
        from avvad import ops
        B, L = case["est"].shape
        wide_e = torch.full((B, L + pad), float("nan"), device=DEV)
        wide_r = torch.full((B, L + pad), float("nan"), device=DEV)
        wide_e[:, :L], wide_r[:, :L] = T_(case["est"]).to(DEV), T_(case["ref"]).to(DEV)
        wide_e.requires_grad_(True)
        loss, ratios = ops.si_sdr_loss(wide_e[:, :L], wide_r[:, :L], case["lengths"], case["head"], case["tail"], return_ratios=True)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and ratios.dtype == torch.float64 and not ratios.requires_grad
        loss.backward()
        assert torch.count_nonzero(wide_e.grad[:, L:]).item() == 0
        impl.last = (loss.detach(), ratios, wide_e.grad[:, :L].clone(), wide_e.detach()[:, :L], wide_r[:, :L])
        return float(loss.detach()), ratios.cpu().numpy(), wide_e.grad[:, :L].cpu().numpy()
    return impl


@pytest.mark.parametrize("head,tail,pad", [(0, 0, 0), (24, 36, 13)])
def test_si_sdr_loss_and_its_gradient(head, tail, pad):
    """Rows of SCORE_CHUNK + 77 and 300 samples, a row whose window is empty and one of length 0, pitches wider than L, NaN
    behind the lengths; the values also against ops.energy_ratios on the same window, bit for bit."""
    from avvad import ops
    P = ops.SCORE_CHUNK + 77
    lengths = [P, 300, min(40, head + tail), 0]
    case = S.sisdr_case(lengths, P, head, tail, seed=21)
    impl = _loss_impl(pad)
    S.check_sisdr(impl, case)
    loss, ratios, grad, est, ref = impl.last
    assert bool(torch.isnan(ratios[2:]).all())
    win = [max(0, n - head - tail) for n in lengths]
    scored = ops.energy_ratios(est[:, head:], ref[:, head:], lengths=win)[:, 0]
    assert torch.equal(ratios[:2], scored[:2])
    total = 0.0
    for v in scored[:2].tolist():
        total += v
    assert float(loss) == float(np.float32(-total))
    # a scaled upstream gradient scales the result; a second run gives the same bits
    again = _loss_impl(pad)
    again(case)
    assert torch.equal(again.last[2], grad) and torch.equal(again.last[0], loss)
    e = est.clone().requires_grad_(True)
    (ops.si_sdr_loss(e, ref, lengths, head, tail) * 0.5).backward()
    assert torch.equal(e.grad, grad * 0.5)


def _chain(case):
    from avvad import ops
    noisy, clean = T_(case["noisy"]).to(DEV), T_(case["clean"]).to(DEV)
    logits = T_(case["mask"]).to(DEV).requires_grad_(True)
    est = ops.resynth(noisy, logits, mask_mode=2, n_fft=case["n_fft"], hop=case["hop"], sample_lengths=case["lengths"])
    loss = ops.si_sdr_loss(est, clean, case["lengths"], case["skip"], case["skip"])
    loss.backward()
    return loss.detach(), logits.grad


def test_chain_from_logits_to_their_gradient():
    """logits -> resynth -> windowed loss -> dlogits at 1024 / 256, B = 2 ragged, against the float64 chain; two runs give
    the same bits"""
    case = S.chain_case(1024, 256, [6000, 4300], seed=31)
    loss, grad = _chain(case)
    S.check_chain(lambda c: (float(loss), grad.cpu().numpy()), case, _report, "chain 1024/256 B = 2")
    loss2, grad2 = _chain(case)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def test_training_on_si_sdr(tmp_path):
    """DeepVAD_audio (513 bins, one layer, hidden 32) on the committed noisy / clean pair, used twice as a batch: Adam at
    1e-3, 8 steps.  The step-8 loss is below the step-1 loss, two runs from the same seed end in the same parameter bits,
    a checkpoint is written and the log line carries the batch's SI-SDR."""
    from avvad import train as TR
    from packages.models.Audio_Net import DeepVAD_audio
    pair = (os.path.join(GOLDEN, "utt_sa1.npz"), os.path.join(GOLDEN, "utt_sa1_clean.npz"))
    states, losses = [], []
    for run in ("a", "b"):
        out = str(tmp_path / run)
        model = TR.train_main("audio", lambda: DeepVAD_audio(1, 32, 513), "sisdr", epochs=8, batch_size=2, lr=1e-3, out_dir=out,
                              wav_pairs=[pair, pair], objective="si_sdr")
        states.append({k: v.detach().clone() for k, v in model.state_dict().items()})
        log = open(os.path.join(out, "output_batch.log")).read()
        steps = re.findall(r"train batch +0  loss (\S+) .* si-sdr (\S+) dB", log)
        assert len(steps) == 8, log
        losses.append([float(a) for a, _ in steps])
        assert all(abs(float(a) + 2 * float(b)) < 0.02 for a, b in steps)            # loss = -(sum of two rows), mean in dB
        assert len([f for f in os.listdir(out) if f.endswith(".pt")]) == 8
    print("sisdr: training loss per step", losses[0])
    assert losses[0][7] < losses[0][0], losses[0]
    assert losses[0] == losses[1]
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k
