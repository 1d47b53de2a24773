"""GPU tests of the mask-regression losses (csrc/spectral_loss.hip, ``ops.spectral_loss``, the three drop-ins of
``packages/models/utils.py`` and the objectives "mse_mask" / "mse_signal" / "msa" of ``train_main``) against the float64
restatement of tests/spectral_loss_ref.py, at the bounds that file derives from its float32 stand-in.

The case list reaches every loop of ``spectral_finish`` past its first trip: "chunks130" (4 x 517 x 513, rows of 130, 65,
64 and 0 chunks: the lane loop over a row's partials runs three trips, two with one chunk in the second, exactly one, none;
``spectral_pass`` runs workgroups with blockIdx.x up to 129) and "rows67" (67 x 7 x 33: five trips of the wave-per-row
loop of 16 waves, two of the 64-lane sum over rows).  Both go through the parametrised value test, through the C ABI with
a NaN-filled workspace, and row by row against the same row alone."""
import ctypes as Ct
import os
import re

import numpy as np
import pytest
import torch

import spectral_loss_ref as R
from conftest import GOLDEN, ROOT
from test_mix_gpu import _files
from test_spectral_loss_cpu import golden_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = int(re.search(r"#define AVVAD_SPECTRAL_CHUNK (\d+)", open(os.path.join(ROOT, "include", "avvad.h")).read()).group(1))


def _ops():
    from avvad import ops
    return ops


def _stream():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _args(c):
    """the keyword arguments of ops.spectral_loss for a case, on the GPU (only what the kind reads)"""
    kw = {"pred_mode": c["pred_mode"], "lengths": None if c["lengths"] is None else list(c["lengths"])}
    if c["kind"] != "spectrum":
        kw["target"] = c["target"].to(DEV)
    if c["kind"] != "mask":
        kw["mix"] = c["mix"].to(DEV)
    if c["kind"] == "spectrum":
        kw["speech"] = c["speech"].to(DEV)
    return kw


def run_ops(c, upstream=None):
    """(loss, rows, dpred) of a case through ops.spectral_loss and autograd, as torch tensors on the GPU"""
    pred = c["pred"].to(DEV).requires_grad_(True)
    loss, rows = _ops().spectral_loss(pred, c["kind"], return_rows=True, **_args(c))
    assert loss.dtype == torch.float32 and loss.shape == () and rows.dtype == torch.float64 and rows.shape == (c["B"],)
    (loss if upstream is None else loss * upstream).backward()
    return loss.detach(), rows, pred.grad


def as_numpy(got):
    return float(got[0]), got[1].cpu().numpy(), got[2].cpu().numpy()


def run_abi(c, want_dpred=True, want_rows=True, shift=0):
    """The same through the C ABI; ``shift``: every float buffer starts that many floats behind a 256-byte boundary (the
    spectra twice as many: their pairs stay on 8 bytes)."""
    from avvad import _lib as L
    lib = L.lib()
    B, T, F = c["B"], c["T"], c["F"]

    def put(t, by):
        flat = torch.empty(t.numel() + by, dtype=torch.float32, device=DEV)
        flat[by:] = t.reshape(-1).to(DEV)
        return flat[by:]
    pred, target = put(c["pred"], shift), put(c["target"], shift)
    mix, speech = put(torch.view_as_real(c["mix"]), 2 * shift), put(torch.view_as_real(c["speech"]), 2 * shift)
    assert pred.data_ptr() % 16 == 4 * shift % 16 and mix.data_ptr() % 16 == 8 * shift % 16
    loss = torch.full((1,), float("nan"), device=DEV)
    rows = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV) if want_rows else None
    dpred = torch.full((B * T * F + shift,), float("nan"), device=DEV)[shift:] if want_dpred else None
    lens = None if c["lengths"] is None else torch.tensor(c["lengths"], dtype=torch.int32).to(DEV)
    ws = torch.full((lib.avvad_spectral_loss_workspace(B, T, F) // 4,), float("nan"), device=DEV)
    k = R.KINDS.index(c["kind"])
    st = (2 * T * F, 2 * F, 2)
    L.check(lib.avvad_spectral_loss(L.ptr(pred), c["pred_mode"], k, L.ptr(target) if k < 2 else None, L.ptr(mix) if k else None, *st,
                                    L.ptr(speech) if k == 2 else None, *st, L.ptr(lens), L.ptr(loss), L.ptr(rows), L.ptr(dpred),
                                    B, T, F, L.ptr(ws), ws.numel() * 4, _stream()), "avvad_spectral_loss")
    return loss[0], rows, None if dpred is None else dpred.view(B, T, F)


@pytest.mark.parametrize("name, kind, pred_mode", R.CASES)
def test_value_rows_and_autograd_gradient_against_float64(name, kind, pred_mode):
    """every case of the list through ``ops.spectral_loss`` with ``requires_grad`` logits (or mask probabilities)"""
    R.check_spectral(lambda c: as_numpy(run_ops(c)), R.case(name, kind, pred_mode))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", ["ragged", "boundary", "three"])
def test_c_abi_run_to_run_without_dpred_and_off_alignment(name, kind):
    """Through the C ABI: the bounds; two runs bit-equal; the bits of ops; dpred = NULL and row_loss = NULL leave the loss
    bits alone; every buffer 4 bytes (the spectra 8) off a 16-byte boundary gives the same bits."""
    for pred_mode in R.MODES:
        c = R.case(name, kind, pred_mode)
        first = run_abi(c)
        R.check_spectral(lambda _: as_numpy(first), c)
        again, ops_way = run_abi(c), run_ops(c)
        for other in (again, ops_way, run_abi(c, shift=1), run_abi(c, shift=3)):
            assert all(torch.equal(a, b) for a, b in zip(first, other))
        bare = run_abi(c, want_dpred=False, want_rows=False)
        assert torch.equal(bare[0], first[0]) and bare[1] is None and bare[2] is None
        assert torch.equal(run_abi(c, want_dpred=False)[1], first[1])


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", ["chunks130", "rows67"])
def test_c_abi_past_64_chunks_and_64_rows(name, kind):
    """The two shapes that turn the finishing loops, through the C ABI with NaN in the workspace and in every output: the
    bounds; two runs bit-equal; the bits of ops; dpred = NULL leaves the loss and row bits alone."""
    c = R.case(name, kind, 2)
    first = run_abi(c)
    R.check_spectral(lambda _: as_numpy(first), c)
    for other in (run_abi(c), run_ops(c)):
        assert all(torch.equal(a, b) for a, b in zip(first, other))
    bare = run_abi(c, want_dpred=False)
    assert torch.equal(bare[0], first[0]) and torch.equal(bare[1], first[1]) and bare[2] is None


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name, picked", [("rows67", (0, 15, 16, 63, 64, 66)), ("chunks130", (0, 1))])
def test_a_row_has_the_same_bits_alone_and_past_64_rows_or_chunks(name, picked, kind):
    """the file header's promise where the finish loops turn: rows on both sides of the 16-wave and 64-lane strides of
    "rows67", and the rows of 130 and 65 chunks of "chunks130", each alone (B = 1) against its batch row"""
    c = R.case(name, kind, 2)
    _, rows, dpred = run_ops(c)
    for b in picked:
        assert R.lens_of(c)[b] > 0
        loss1, rows1, dpred1 = run_ops(R.single_row(c, b))
        assert torch.equal(rows1[0], rows[b]) and torch.equal(dpred1[0], dpred[b]), (name, kind, b)
        assert float(loss1) == float(np.float32(float(rows[b])))


@pytest.mark.parametrize("kind", ["signal", "spectrum"])
def test_spectrum_layouts_are_read_in_place_with_equal_bits(kind):
    """one utterance with its spectra as (B, T, F, 2), as the transposed legacy (F, T, 2) view and as a complex (F, T)
    tensor: no copy is made and every result has the same bits"""
    ops = _ops()
    c = R.single_row(R.case("ragged", kind, 2), 1)
    T, F = c["T"], c["F"]
    pred, y = c["pred"][0].to(DEV), c["target"][0].to(DEV)
    forms = {}
    for key in ("mix", "speech"):
        z = c[key][0].to(DEV)                                               # complex (T, F)
        ft2 = torch.view_as_real(z).permute(1, 0, 2).contiguous()           # the legacy (F, T, 2) layout
        ft = z.transpose(0, 1).contiguous()                                 # a complex (F, T) tensor
        forms[key] = (torch.view_as_real(z)[None], ft2.permute(1, 0, 2), ft.transpose(0, 1))
        assert forms[key][1].stride() == (2, 2 * T, 1) and not forms[key][2].is_contiguous()
        for v in forms[key]:
            assert ops._spectrum_view(v, key)[0].data_ptr() == v.data_ptr()
    got = []
    for i in range(3):
        p = (pred[None] if i == 0 else pred).clone().requires_grad_(True)
        kw = dict(target=(y[None] if i == 0 else y), mix=forms["mix"][i], lengths=[c["lengths"][0]], return_rows=True)
        if kind == "spectrum":
            kw.update(target=None, speech=forms["speech"][i])
        loss, rows = ops.spectral_loss(p, kind, **kw)
        loss.backward()
        got.append((loss.detach(), rows, p.grad.reshape(1, T, F)))
    R.check_spectral(lambda _: as_numpy(got[0]), c)
    for other in got[1:]:
        assert all(torch.equal(a, b) for a, b in zip(got[0], other))


@pytest.mark.parametrize("kind", R.KINDS)
def test_saturated_logits_give_a_finite_loss_and_no_gradient(kind):
    """rows of nothing but +-30 and +-100: sigmoid is 0 or 1 to float32, the loss is the float64 one, the gradient is zero
    at +-100 and at +30 and below 1e-11 at -30 (m (1 - m) = 9.4e-14 there), nothing is NaN"""
    c = dict(R.case("small", kind, 2))
    vals = torch.tensor([30.0, -30.0, 100.0, -100.0, 100.0])
    c.update(name="all_saturated", pred=vals.repeat(c["B"], c["T"], 1).contiguous())
    loss, rows, dpred = as_numpy(run_ops(c))
    ref_loss, ref_rows, _ = R._reference(c)
    assert np.isfinite(loss) and np.isfinite(rows).all() and np.isfinite(dpred).all()
    assert abs(loss - ref_loss) <= R.BOUND_LOSS * abs(ref_loss) and (np.abs(rows - ref_rows) <= R.BOUND_ROWS * np.abs(ref_rows)).all()
    assert not dpred[..., [0, 2, 3, 4]].any() and np.abs(dpred[..., 1]).max() < 1e-11


@pytest.mark.parametrize("kind", R.KINDS)
def test_a_row_has_the_same_bits_alone_and_in_a_batch_of_five(kind):
    c = R.case("batch5", kind, 2)
    _, rows, dpred = run_ops(c)
    for b in range(c["B"]):
        loss1, rows1, dpred1 = run_ops(R.single_row(c, b))
        assert torch.equal(rows1[0], rows[b]) and torch.equal(dpred1[0], dpred[b]), (kind, b)
        assert float(loss1) == float(np.float32(float(rows[b])))


def test_backward_scales_by_the_upstream_gradient():
    c = R.case("ragged", "spectrum", 2)
    unit, scaled = run_ops(c), run_ops(c, upstream=-2.5)
    assert torch.equal(unit[0], scaled[0]) and torch.equal(scaled[2], unit[2] * torch.tensor(-2.5, device=DEV))
    assert bool((scaled[2][1, 4:] == 0).all()) and bool(scaled[2][0].abs().max() > 0)
    # target, mix and speech are data: no gradient reaches them, and without a gradient to compute none is kept
    ops = _ops()
    y = c["target"].to(DEV).requires_grad_(True)
    loss = ops.spectral_loss(c["pred"].to(DEV).requires_grad_(True), "mask", target=y, lengths=list(c["lengths"]))
    loss.backward()
    assert y.grad is None
    with torch.no_grad():
        assert torch.equal(ops.spectral_loss(c["pred"].to(DEV), "mask", target=y, lengths=list(c["lengths"])), loss.detach())


def test_ops_refuses_mismatched_arguments():
    from avvad import _lib as L
    ops = _ops()
    pred, y = torch.zeros(2, 3, 5, device=DEV), torch.zeros(2, 3, 5, device=DEV)
    z = torch.zeros(2, 3, 5, dtype=torch.complex64, device=DEV)
    for bad in (dict(kind="mask"), dict(kind="mask", target=y[:, :2]), dict(kind="mask", target=y.double()), dict(kind="mask", target=y.cpu()),
                dict(kind="signal", target=y), dict(kind="signal", target=y, mix=z[:1]), dict(kind="signal", target=y, mix=z.to(torch.complex128)),
                dict(kind="spectrum", mix=z), dict(kind="spectrum", mix=z, speech=z[:, :, :4]), dict(kind="mask", target=y, lengths=[3]),
                dict(kind="mask", target=y, pred_mode=3)):
        with pytest.raises(L.AvvadError):
            ops.spectral_loss(pred, **bad)
    for bad_pred in (pred.double(), pred[0, 0], pred.cpu()):
        with pytest.raises(L.AvvadError):
            ops.spectral_loss(bad_pred, "mask", target=y)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_drop_ins_against_the_recorded_reference(tag):
    """the three functions of packages/models/utils.py on the recorded utterances: the reference's own values, and the
    gradient in y_hat against float64"""
    from packages.models import utils as U
    for kind in R.KINDS:
        c, want = golden_case(tag, kind)
        y_hat = c["pred"][0].to(DEV).requires_grad_(True)
        x, s, y = c["mix"][0].to(DEV), c["speech"][0].to(DEV), c["target"][0].to(DEV)
        if kind == "mask":
            loss = U.mean_square_error_mask(y, y_hat)
        elif kind == "signal":
            loss = U.mean_square_error_signal(x, y, y_hat)
            assert abs(float(U.mean_square_error_signal(x.abs(), y, y_hat.detach())) - want) <= R.BOUND_LOSS * want   # x a magnitude
        else:
            loss = U.magnitude_spectrum_approxiamation_loss(x, s, y_hat)
        loss.backward()
        value = float(loss.detach())
        print("%s %-8s %.9g (reference %.9g)" % (tag, kind, value, want))
        assert abs(value - want) <= R.BOUND_LOSS * abs(want), (kind, value, want)
        R.check_spectral(lambda _: (value, np.array([value]), y_hat.grad.cpu().numpy()[None]), c)


def _train(tmp_path, objective, mixing):
    from avvad import train as TR
    from packages.models.Audio_Net import DeepVAD_audio
    kw = dict(epochs=3, batch_size=2, lr=1e-2, objective=objective)
    if mixing:
        _files(tmp_path)
        kw.update(clean_wavs=str(tmp_path / "clean.txt"), noise_wavs=str(tmp_path / "noise.txt"), snr_db=5.0, mix_seed=4,
                  mix_labels="irm")
    else:
        pair = (os.path.join(GOLDEN, "utt_sa1.npz"), os.path.join(GOLDEN, "utt_sa1_clean.npz"))
        kw.update(wav_pairs=[pair, pair])
    states, losses = [], []
    for run in ("a", "b"):
        out = str(tmp_path / run)
        model = TR.train_main("audio", lambda: DeepVAD_audio(1, 32, 513), "spectral", out_dir=out, **kw)
        states.append({k: v.detach().clone() for k, v in model.state_dict().items()})
        log = open(os.path.join(out, "output_batch.log")).read()
        train = [float(v) for v in re.findall(r"train loss (\S+)", log)]
        valid = [float(v) for v in re.findall(r"valid loss (\S+)", log)]
        assert len(train) == len(valid) == 3 and all(np.isfinite(train + valid)), log
        assert len(re.findall(r"train batch +0 .* %s/utt \S+" % objective, log)) == 3, log
        assert len([f for f in os.listdir(out) if f.endswith(".pt")]) == 3
        losses.append(train)
    print("%s%s: training loss per epoch %s" % (objective, " (mixed, irm)" if mixing else "", losses[0]))
    assert losses[0][2] < losses[0][0], losses[0]
    assert losses[0] == losses[1]
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k


@pytest.mark.parametrize("objective, mixing", [("mse_mask", False), ("mse_signal", False), ("msa", False), ("msa", True)])
def test_training_on_the_mask_regression_objectives(tmp_path, objective, mixing):
    """DeepVAD_audio (513 bins, one layer, hidden 32), Adam, 3 epochs of one step: on the committed noisy / clean pair used
    twice as a batch, and for "msa" once more on two clean crops mixed with noise in the step with the IRM as the label.
    Finite losses, the third training loss below the first, two runs from the same seeds end in the same parameter bits."""
    _train(tmp_path, objective, mixing)
