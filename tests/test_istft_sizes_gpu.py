"""The masked inverse STFT, its adjoint and the SI-SDR loss on the GPU past the sizes of tests/test_istft_gpu.py and
tests/test_sisdr_gpu.py: past one trip (``istft_sizes_ref.TRIP`` elements) of the grid-stride loops overlap_add,
overlap_add_adjoint and mask_gradient, at 4160 GEMM rows in 33 x 8 tiles (the small tests stop at row 259 and 24 tiles),
under a launch plan of data-parallel rounds plus a split remainder, and over more rows than the loss's one workgroup
(256) and gram_finalize's (64) take in one stride.

References and bounds are those of the small tests, unchanged: ``istft_ref.FACTOR x E_cpu32`` of the same input for every
GEMM result, ``check_sisdr``'s 1e-6 dB and ``GRAD_EPS`` for the loss, ``test_score_gpu.TOL_DB`` for the ratios.  Observed
error and bound of every case go to the parity log.  tests/test_istft_sizes_cpu.py proves on the CPU that a kernel which
stops after one trip, or takes its second trip from an index that is off by one row, fails these checks."""
import numpy as np
import pytest
import torch

import istft_ref as R
import istft_sizes_ref as Z
import sisdr_ref as S
from test_gpu_parity import _report as _parity_report
from test_score_gpu import TOL_DB
from test_sisdr_gpu import _istft_grad, _loss_impl

pytestmark = pytest.mark.gpu
T_ = torch.from_numpy
DEV = "cuda:0"


def _report_istft(name, got, ref, atol):
    _parity_report("istft: " + name, got, ref, atol)


def _report_sisdr(name, got, ref, atol):
    _parity_report("sisdr: " + name, got, ref, atol)


def _forward(case):
    """ops.istft on the case's NaN-padded buffers -> (B, pitch) tensor"""
    from avvad import ops
    kw = dict(mask=T_(case["logits"]).to(DEV), mask_mode=2) if case["mode"] == 2 else {}
    out = ops.istft(T_(case["spec"]).to(DEV), case["n_fft"], case["hop"], n_frames=case["frames"], center=case["center"], **kw)
    assert out.dtype == torch.float32 and out.shape == (len(case["frames"]), case["pitch"])
    return out


@pytest.mark.parametrize("center,mode", [(False, 0), (True, 0), (False, 2)])
def test_batched_forward_past_one_trip_of_overlap_add(center, mode):
    """16 ragged rows at 1024 / 256 (``FRAMES``), NaN in the padding frames: B pitch = 1 077 248 (centred 1 060 864)
    output elements, so overlap_add's second trip is row 15 from sample 38 656 (centred: its last 12 288 samples), and
    B T = 4160 GEMM rows take MaskedSpec's (b, t) arithmetic to x = 4159.  Every row under ``_check_row``'s rule, exact
    zeros behind each row's length; mode 2 against the float64-masked spectrum."""
    case = Z.forward_case(Z.N_FFT, Z.HOP, Z.FRAMES, center, mode, seed=7)
    assert case["frames"][15] == max(case["frames"]) == 260 and 15 * case["pitch"] < Z.TRIP < 16 * case["pitch"]
    assert case["pitch"] == (66304 if center else 67328)
    assert np.count_nonzero(Z.reference_past_trip(case, 15)) == 16 * case["pitch"] - Z.TRIP     # compared, and not against zeros
    out = _forward(case).cpu().numpy()
    Z.check_forward(out, case, _report_istft, "sizes 1024/256 B=16 center %d mode %d" % (center, mode))


@pytest.mark.parametrize("n_fft,hop,T", Z.LONG)
def test_one_long_utterance_past_one_trip(n_fft, hop, T):
    """B = 1: 65 600 frames at 64 / 16 (L = 1 049 648; 513 x 1 GEMM tiles: one data-parallel round of 512 and one tile
    split three ways) and 4100 frames at 1024 / 256 (L = 1 050 368): the samples from 1 048 576 on belong to overlap_add's
    second trip, are compared, and their reference is not zero."""
    from avvad import ops
    case = Z.forward_case(n_fft, hop, (T,), False, 0, seed=n_fft + hop)
    assert case["pitch"] == n_fft + hop * (T - 1) > Z.TRIP
    tail = Z.reference_past_trip(case, 0)
    assert tail.size == case["pitch"] - Z.TRIP and np.count_nonzero(tail) == tail.size
    out = ops.istft(T_(case["spec"]).to(DEV), n_fft, hop)
    assert out.shape == (1, case["pitch"])
    Z.check_forward(out.cpu().numpy(), case, _report_istft, "sizes %d/%d one row of %d frames" % (n_fft, hop, T))


def test_forward_as_full_rounds_plus_a_split_remainder(lib_options):
    """The batch of the first test under two launch plans of igemm::launch<128, 128> (csrc/igemm.h, csrc/streamk.h).  The
    product has cdiv(4160, 128) x cdiv(1024, 128) = 33 x 8 = 264 tiles of ktiles = cdiv(1028, 32) = 33 K tiles; the 8-wave
    kernel keeps 2 workgroups per CU, so ``workers()`` gives G = 2 x 256 = 512.
    * default: 264 < 512, so plan_rounds leaves full_rounds = 0 and rem = 264 -- every tile in the stream-K pool of
      264 x 33 = 8712 iterations on 512 workers (the cap iterations / 4 = 2178 does not bind), fix-up by fixup1;
    * ``max_cus`` = 64: G = 128, full_rounds = 264 / 128 = 2, rem = 8 (8 x 10 < 128 x 9, so the remainder stays split):
      256 tiles in two data-parallel rounds, then 8 tiles = 264 iterations cut between 128 workers, fix-up by the
      four-wave kernel (16 slabs per tile).
    Both meet the float64 bound.  Bits may differ between the plans (a tile's K range is cut elsewhere); under one plan two
    runs give the same bits."""
    case = Z.forward_case(Z.N_FFT, Z.HOP, Z.FRAMES, False, 0, seed=7)
    outs = []
    for name, cus in (("default plan", None), ("max_cus 64", 64)):
        if cus is not None:
            lib_options("max_cus", cus)
        first, again = _forward(case), _forward(case)
        assert torch.equal(first, again), name
        Z.check_forward(first.cpu().numpy(), case, _report_istft, "sizes 1024/256 B=16 " + name)
        outs.append(first)
    print("istft: samples whose bits differ between the two plans: %d of %d" % (int((outs[0] != outs[1]).sum()), outs[0].numel()))


def test_basis_kernels_past_several_trips():
    """n_fft = 2048: idft_basis writes 2052 x 2048 = 4 202 496 elements and the forward transform's basis as many -- four
    whole trips and a fifth begun, where 1024 passes the first trip by two non-zero rows.  The forward and the adjoint (whose
    GEMM reads the forward basis) on a ragged batch of (3, 1) frames at hop 512."""
    n_fft, hop, frames = 2048, 512, (3, 1)
    assert (2 * (n_fft // 2 + 1) + 3) // 4 * 4 * n_fft > 4 * Z.TRIP
    case = Z.forward_case(n_fft, hop, frames, False, 0, seed=9)
    Z.check_forward(_forward(case).cpu().numpy(), case, _report_istft, "sizes 2048/512")
    adj = S.cached_istft_case(n_fft, hop, frames, 2, True, 10)
    S.check_dmask(_istft_grad, adj, _report_sisdr, "sizes 2048/512 adjoint")


@pytest.mark.parametrize("which", ["A", "B"])
def test_batched_adjoint_past_one_trip(which):
    """dmask of the 16-row batch: mask_gradient runs over 16 x 260 x 513 = 2 134 080 elements (two trips and a third begun),
    overlap_add_adjoint over 16 x 67 328 = 1 077 248 (its second trip is q[15] from sample 38 656 on, seen through row 15 of
    dmask only -- hence the long last row), framed_dft over 33 x 9 tiles.  A: logits, not centred.  B: a mask, centred, a
    scale per row, rows 6 and 15 cut below their natural length."""
    case = Z.adjoint_case(which)
    assert case["frames"][15] == 260 and case["ref"].size == 2134080
    tail = Z.past_trip(case["ref"])
    assert tail.size == 1085504 and 2 * np.count_nonzero(tail) >= tail.size
    assert np.count_nonzero(case["ref"][15]) * 2 >= case["ref"][15].size
    S.check_dmask(_istft_grad, case, _report_sisdr, "sizes 1024/256 B=16 adjoint " + which)


def test_adjoint_of_a_row_without_frames():
    """n_frames = 0 in the middle of a batch: the row's dmask is exactly zero and nothing of its NaN padding is read"""
    case = S.cached_istft_case(64, 16, (9, 0, 4), 2, True, 5)
    assert case["lengths"][1] == 0 and not case["ref"][1].any()
    S.check_dmask(_istft_grad, case, _report_sisdr, "istft 64/16 a row of 0 frames")


def _chain(case, fused, spec=None):
    """logits -> est -> windowed SI-SDR loss -> dlogits, through ops.resynth or through ops.istft on ``spec``"""
    from avvad import ops
    noisy, clean = T_(case["noisy"]).to(DEV), T_(case["clean"]).to(DEV)
    logits = T_(case["mask"]).to(DEV).requires_grad_(True)
    if fused:
        est = ops.resynth(noisy, logits, mask_mode=2, n_fft=case["n_fft"], hop=case["hop"], sample_lengths=case["lengths"])
    else:
        est = ops.istft(spec, case["n_fft"], case["hop"], mask=logits, mask_mode=2, n_frames=case["frames"], length=case["lengths"])
    loss = ops.si_sdr_loss(est, clean, case["lengths"], case["skip"], case["skip"])
    loss.backward()
    return loss.detach(), logits.grad, est.detach()


def test_chain_at_a_training_steps_shape():
    """16 utterances of 3 s (two shorter) at 1024 / 256: 185 frames, B T F = 1 518 480 elements of mask_gradient.  dlogits
    against the float64 chain, the same bits from two runs, and the fused backward equal to ops.stft_complex -> ops.istft's
    bit for bit."""
    from avvad import ops
    case = Z.chain_case()
    assert case["mask"].size == 1518480 > Z.TRIP and np.count_nonzero(Z.past_trip(case["ref"])) * 2 >= case["mask"].size - Z.TRIP
    loss, grad, est = _chain(case, True)
    S.check_chain(lambda c: (float(loss), grad.cpu().numpy()), case, _report_sisdr, "sizes chain 1024/256 B=16")
    loss2, grad2, est2 = _chain(case, True)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2) and torch.equal(est, est2)
    spec = ops.stft_complex(T_(case["noisy"]).to(DEV), case["n_fft"], case["hop"])
    assert spec.shape == case["mask"].shape + (2,)
    loss3, grad3, est3 = _chain(case, False, spec)
    assert torch.equal(est, est3) and torch.equal(loss, loss3) and torch.equal(grad, grad3)


def test_si_sdr_loss_and_ratios_over_300_rows():
    """B = 300 > the 256 threads of sisdr_coefficients' one workgroup and > the 64 rows of a gram_finalize workgroup; the row
    of SCORE_CHUNK + 77 samples, the empty window and the zero length all sit at rows >= 256.  The loss under
    ``check_sisdr``, its float32 value equal to the rounded negated sum of ops.energy_ratios' values in ascending row order,
    and ops.energy_ratios with the noise on the same rows against float64."""
    from avvad import ops
    case = Z.loss_case(ops.SCORE_CHUNK)
    lengths, head, tail = case["lengths"], case["head"], case["tail"]
    assert min(Z.LOSS_EMPTY_WINDOW, Z.LOSS_ZERO_LENGTH, Z.LOSS_LONG) >= 256 and lengths[Z.LOSS_LONG] > ops.SCORE_CHUNK
    impl = _loss_impl(13)
    S.check_sisdr(impl, case, name="si_sdr_loss B=300")
    loss, ratios, grad, est, ref = impl.last
    win = [max(0, n - head - tail) for n in lengths]
    live = [b for b, n in enumerate(win) if n > 0]
    assert len(live) == Z.LOSS_B - 2 and bool(torch.isnan(ratios[[Z.LOSS_EMPTY_WINDOW, Z.LOSS_ZERO_LENGTH]]).all())
    _report_sisdr("si_sdr_loss B=300 ratios (dB)", ratios[live].cpu().numpy(), case["ref64"][1][live], 1e-6)
    _, _, _, c1, c2 = S.sisdr_closed(case["est"], case["ref"], lengths, head, tail)
    mag = np.abs(c1[:, None] * np.nan_to_num(case["ref"]).astype(np.float64)) + np.abs(c2[:, None] * np.nan_to_num(case["est"]).astype(np.float64))
    inside = case["ref64"][2] != 0
    _report_sisdr("si_sdr_loss B=300 gradient / (|c1 s| + |c2 e|)", grad.cpu().numpy()[inside] / mag[inside],
                  case["ref64"][2][inside] / mag[inside], S.GRAD_EPS)
    scored = ops.energy_ratios(est[:, head:], ref[:, head:], lengths=win)[:, 0]
    assert torch.equal(ratios[live], scored[live])
    total = 0.0
    for v in scored[live].tolist():
        total += v
    assert float(loss) == float(np.float32(-total))
    again = _loss_impl(13)
    again(case)
    assert torch.equal(again.last[0], loss) and torch.equal(again.last[2], grad)
    # the three ratios of the whole rows, with the noise
    got = ops.energy_ratios(T_(case["est"]).to(DEV), T_(case["ref"]).to(DEV), noise=T_(case["noise"]).to(DEV), lengths=lengths)
    assert got.shape == (Z.LOSS_B, 3) and got.dtype == torch.float64
    got = got.cpu().numpy()
    rows = [b for b, n in enumerate(lengths) if n > 0]
    assert np.isnan(got[Z.LOSS_ZERO_LENGTH]).all() and len(rows) == Z.LOSS_B - 1
    _report_sisdr("energy_ratios B=300 (dB)", got[rows], case["ratios64"][rows], TOL_DB)
