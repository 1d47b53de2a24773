"""The caller-owned buffer contract of include/avvad.h for the scores (avvad_score_accumulate, avvad_score_finalize,
avvad_confusion_accumulate), through tests/abi_guard.py as tests/test_istft_stream_contract_gpu.py does for its family:
zero-, NaN- and 1e30-filled guarded workspaces give the same bits with the guards intact; a workspace one float short is
refused (AVVAD_EWORKSPACE) with everything still poisoned; a workspace 4 bytes off its alignment, an accumulator or a
counts array 4 bytes off its 8-byte alignment and a row pitch below L are refused (AVVAD_EINVAL) before anything is
launched."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import score_ref
from abi_guard import expect_refused, run_contract

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
T_ = torch.from_numpy


def _ops():
    from avvad import ops
    return ops


def _stream():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ragged():
    """B = 3 rows of pitch C + 77 with lengths [C + 77, 300, 0], NaN behind the lengths."""
    P = _ops().SCORE_CHUNK + 77
    lengths = [P, 300, 0]
    rows = [score_ref.mix(np.random.default_rng(31), P, 0.1, 20.0), score_ref.mix(np.random.default_rng(32), 300, 1.0, 0.0), None]
    sig = [np.full((3, P), NAN, dtype=np.float32) for _ in range(3)]
    for b, r in enumerate(rows):
        for j in range(3):
            if r is not None:
                sig[j][b, :lengths[b]] = r[j]
    return lengths, rows, [T_(x).to(DEV) for x in sig]


def test_scores_with_poisoned_buffers(monkeypatch):
    ops = _ops()
    lengths, rows, (ed, sd, nd) = _ragged()

    def case():
        ratios, alpha = ops.energy_ratios(ed, sd, noise=nd, lengths=lengths, return_alpha=True)
        mix = ops.energy_ratios(ed, sd, mixture=nd, lengths=lengths)
        # (row 2 is NaN: compared as bits)
        return {"ratios": ratios.view(torch.int64), "alpha": alpha.view(torch.int64), "mixture": mix.view(torch.int64)}
    got = run_contract(monkeypatch, ops, case)
    ratios = got["ratios"].view(torch.float64).cpu().numpy()
    for b in (0, 1):
        want = np.array(score_ref.energy_ratios(*rows[b]))
        assert np.all((want >= -10) & (want <= 60)) and np.abs(ratios[b] - want).max() <= 1e-6
    assert np.isnan(ratios[2]).all()
    # the workspace 4 bytes off its alignment
    expect_refused(monkeypatch, ops, case, "AVVAD_EINVAL", offset=1)


def test_misaligned_accumulators_and_short_pitches_are_refused():
    """Through the C ABI: acc / counts 4 bytes off their 8-byte alignment and a pitch below L return AVVAD_EINVAL and
    nothing has changed; the same calls with proper arguments succeed."""
    from avvad import _lib as L
    ops = _ops()
    lib = L.lib()
    off4 = lambda t: Ct.c_void_p(t.data_ptr() + 4)          # noqa: E731
    n = 300
    e, s, v = (T_(x).to(DEV) for x in score_ref.mix(np.random.default_rng(33), n, 0.1, 20.0))
    acc = torch.zeros(1, 8, dtype=torch.float64, device=DEV)                # room for the shifted pointer
    ws = torch.full((lib.avvad_score_workspace(1, n) // 4,), NAN, device=DEV)

    def accumulate(acc_p, ld_e=n, ld_s=n, ld_v=n):
        return lib.avvad_score_accumulate(L.ptr(e), ld_e, L.ptr(s), ld_s, L.ptr(v), ld_v, 1, None, acc_p, 1, n, L.ptr(ws),
                                          ws.numel() * 4, _stream())
    for rc in (accumulate(off4(acc)), accumulate(L.ptr(acc), ld_e=n - 1), accumulate(L.ptr(acc), ld_s=n - 1),
               accumulate(L.ptr(acc), ld_v=n - 1)):
        assert rc == -1
        assert torch.count_nonzero(acc).item() == 0 and bool(torch.isnan(ws).all())
    assert accumulate(L.ptr(acc)) == 0
    ratios = torch.full((1, 4), NAN, dtype=torch.float64, device=DEV)
    assert lib.avvad_score_finalize(off4(acc), 1, 1, L.ptr(ratios), None, _stream()) == -1
    assert lib.avvad_score_finalize(L.ptr(acc), 1, 1, off4(ratios), None, _stream()) == -1
    assert bool(torch.isnan(ratios).all())
    assert lib.avvad_score_finalize(L.ptr(acc), 1, 1, L.ptr(ratios), None, _stream()) == 0
    want = np.array(score_ref.energy_ratios(e.cpu().numpy(), s.cpu().numpy(), v.cpu().numpy()))
    assert np.abs(ratios[0, :3].cpu().numpy() - want).max() <= 1e-6 and bool(torch.isnan(ratios[0, 3]))
    assert torch.count_nonzero(acc[0, 6:]).item() == 0
    # the counts
    pred = (torch.rand(2, 5, 3, device=DEV) > 0.5).float()
    target = (torch.rand(2, 5, 3, device=DEV) > 0.5).float()
    counts = torch.zeros(9, dtype=torch.int64, device=DEV)
    assert lib.avvad_confusion_accumulate(L.ptr(pred), 0, L.ptr(target), None, off4(counts), 2, 5, 3, _stream()) == -1
    assert torch.count_nonzero(counts).item() == 0
    assert lib.avvad_confusion_accumulate(L.ptr(pred), 0, L.ptr(target), None, L.ptr(counts), 2, 5, 3, _stream()) == 0
    assert counts[:8].view(2, 4).sum(dim=1).tolist() == [15, 15] and int(counts[8]) == 0
    assert torch.equal(counts[:8].view(2, 4), ops.confusion_counts(pred, target))
