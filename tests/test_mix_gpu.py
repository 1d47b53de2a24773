"""The SNR mix on the GPU (csrc/mix.hip through ``ops.mix``) against the float64 reference and the bounds of
tests/mix_ref.py: a ragged batch whose row and clip lengths reach every branch of the circular read (rows of 0, 1, 255,
4095, 4096, 4097 and 3 * 4096 + 17 samples; clips of 1, 255, 4096, 5000 samples, one as long as its row, a 300-sample
clip under a 9000-sample row), SNRs of -20, 0, 7.5 and 40 dB, B = 1, 12, 33 and 70 (``mix_gain`` takes one thread per
row in workgroups of 64: the 70-row case is the one that launches its second workgroup), every base pointer 4 bytes off a 16-byte
boundary, NaN behind every row's length, degenerate rows; equal bits from run to run, for a row alone and under a CU cap;
then the chain (``mix_step`` on the committed clean utterance) and two short trainings on mixtures made in the step."""
import os
import re

import numpy as np
import pytest
import torch

import mix_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
MARK = 7.0               # what the wider output tensors hold outside the columns the mix owns


def _ops():
    from avvad import ops
    return ops


def _off4(rows, cols, fill):
    """(wide, view): a (rows, cols) column slice of a wider tensor whose base lies 4 bytes behind a 16-byte boundary"""
    wide = torch.full((rows, (cols + 1 + 3) // 4 * 4 + 4), fill, dtype=torch.float32, device=DEV)
    view = wide[:, 1:1 + cols]
    assert view.data_ptr() % 16 == 4 and (wide.stride(0) * 4) % 16 == 0
    return wide, view


_BANK = {}


def _bank():
    """the shared clips as a NoiseBank whose flat buffer starts 4 bytes behind a 16-byte boundary"""
    if "bank" not in _BANK:
        ops = _ops()
        bank = ops.NoiseBank([torch.from_numpy(c) for c in mix_ref.clips()], DEV)
        wide, view = _off4(1, bank.data.numel(), NAN)
        view[0].copy_(bank.data)
        bank.data = view[0]
        _BANK["bank"] = (bank, wide)
    return _BANK["bank"][0]


def _device_case(case):
    """clean on the GPU: a 4-byte-off slice, NaN behind every row's length and around the rows"""
    wide, clean = _off4(case["clean"].shape[0], case["L"], NAN)
    host = case["clean"].copy()
    for b, n in enumerate(case["lengths"]):
        host[b, n:] = NAN
    clean.copy_(torch.from_numpy(host))
    return wide, clean


def _mix(case, info=True):
    """ops.mix on a case with every pointer off its 16 bytes -> (noisy, noise, info, the two wide output tensors)"""
    ops = _ops()
    _, clean = _device_case(case)
    B, L = clean.shape
    wide_y, y = _off4(B, L, MARK)
    wide_z, z = _off4(B, L, MARK)
    got = ops.mix(clean, case["lengths"], _bank(), case["clip"], case["start"], case["snr_db"], return_info=info, out=y, noise_out=z)
    assert got[0].data_ptr() == y.data_ptr() and got[1].data_ptr() == z.data_ptr()
    return y, z, (got[2] if info else None), wide_y, wide_z


def _impl(case):
    y, z, info, wide_y, wide_z = _mix(case)
    ops = _ops()
    L = case["L"]
    for wide in (wide_y, wide_z):                    # the columns the mix does not own are as they were
        assert bool((wide[:, 0] == MARK).all()) and bool((wide[:, 1 + L:] == MARK).all())
    assert torch.equal(info["peak"].view(torch.int32), ops.peak(y.contiguous()).view(torch.int32))
    return {"noisy": y.cpu().numpy(), "noise": z.cpu().numpy(), "gain": info["gain"].cpu().numpy(),
            "energies": info["energies"].cpu().numpy(), "peak": info["peak"].cpu().numpy()}


def _bits(*ts):
    return [t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64).clone() for t in ts]


def _all_bits(case):
    y, z, info, _, _ = _mix(case)
    return _bits(y, z, info["gain"], info["energies"], info["peak"])


@pytest.mark.parametrize("name", ["ragged", "wide"])
def test_ragged_batch_meets_the_bounds(name):
    got = mix_ref.check_named(_impl, name)
    case = mix_ref.ragged_case() if name == "ragged" else mix_ref.wide_case()
    for b in range(len(case["lengths"])):
        degenerate = (b % len(mix_ref.ROWS)) in mix_ref.DEGENERATE
        assert (got["gain"][b] == 0.0) == degenerate
    print("%s: gains %s" % (name, got["gain"][:12]))


def test_seventy_rows_reach_the_second_gain_workgroup(lib_options):
    """B = 70 ("wide70"): the bounds with 4-byte-off pointers and NaN tails; a zero gain exactly on the degenerate rows;
    two runs bit-equal; rows 63, 64 and 69 alone equal their batch rows; equal bits under a cap of 8 CUs."""
    from avvad import _lib as L
    case = mix_ref.wide70_case()
    got = mix_ref.check_named(_impl, "wide70")
    assert len(case["lengths"]) == 70
    for b in range(70):
        assert (got["gain"][b] == 0.0) == ((b % len(mix_ref.ROWS)) in mix_ref.DEGENERATE), b
    print("wide70: gains of rows 60 .. 69 %s" % got["gain"][60:])
    first, second = _all_bits(case), _all_bits(case)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    for b in (63, 64, 69):
        for whole, one in zip(first, _all_bits(mix_ref.single_row(case, b))):
            assert torch.equal(whole[b:b + 1], one), b
    default = L.get_option("max_cus")
    lib_options("max_cus", 8)
    capped = _all_bits(case)
    lib_options("max_cus", default)
    for a, b in zip(first, capped):
        assert torch.equal(a, b)


def test_plain_call_returns_new_tensors():
    """without out / noise_out and without lengths: contiguous results, one value unless more is asked for; a 1-D wave"""
    ops = _ops()
    case = mix_ref.single_row(mix_ref.ragged_case(), 6)
    n = case["lengths"][0]
    clean = torch.from_numpy(case["clean"][:, :n].copy()).to(DEV)
    y = ops.mix(clean, None, _bank(), case["clip"], case["start"], case["snr_db"])
    assert isinstance(y, torch.Tensor) and y.shape == (1, n) and y.is_contiguous()
    y1, z1, info = ops.mix(clean[0], [n], _bank(), case["clip"], case["start"], case["snr_db"][0], return_noise=True, return_info=True)
    assert y1.shape == z1.shape == (n,) and torch.equal(y1, y[0]) and set(info) == {"gain", "energies", "peak"}
    assert torch.equal(y1, clean[0] + z1)                    # the sum is not contracted: noisy - clean is the noise handed out
    whole = _mix(mix_ref.ragged_case())[0]
    assert torch.equal(whole[6, :n], y1)


def test_two_runs_give_equal_bits_and_a_row_alone_equals_its_batch_row():
    case = mix_ref.ragged_case()
    first, second = _all_bits(case), _all_bits(case)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    for b in range(len(case["lengths"])):                    # B = 1
        for whole, one in zip(first, _all_bits(mix_ref.single_row(case, b))):
            assert torch.equal(whole[b:b + 1], one), b


def test_equal_bits_under_a_cu_cap(lib_options):
    from avvad import _lib as L
    case = mix_ref.wide_case()
    default = L.get_option("max_cus")
    free = _all_bits(case)
    lib_options("max_cus", 8)
    capped = _all_bits(case)
    lib_options("max_cus", default)
    again = _all_bits(case)
    for a, b, c in zip(free, capped, again):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_host_validation():
    ops = _ops()
    L = ops.L
    bank = _bank()
    clean = torch.zeros(2, 64, device=DEV)
    ok = dict(lengths=[64, 10], clip=[0, 3], start=[0, 4999], snr_db=[0.0, 5.0])

    def call(**kw):
        a = dict(ok, **kw)
        return ops.mix(clean, a["lengths"], bank, a["clip"], a["start"], a["snr_db"])
    assert call().shape == (2, 64)
    assert call(clip=torch.tensor([0, 3]), start=torch.tensor([0, 1]), snr_db=torch.tensor([0.0, 1.0])).shape == (2, 64)
    for bad in (dict(clip=[0, bank.K]), dict(clip=[-1, 0]), dict(clip=[0]), dict(start=[1, 0]), dict(start=[0, 5000]),
                dict(start=[0, -1]), dict(start=[0, 0, 0]), dict(snr_db=[0.0, NAN]), dict(snr_db=[0.0, float("inf")]),
                dict(snr_db=[0.0]), dict(snr_db=[0.0, 4000.0]), dict(lengths=[64, 65]), dict(lengths=[64])):
        with pytest.raises(L.AvvadError):
            call(**bad)
    with pytest.raises(L.AvvadError, match="NoiseBank"):
        ops.mix(clean, None, [torch.ones(4, device=DEV)], [0, 0], [0, 0], 0.0)
    with pytest.raises(L.AvvadError):
        ops.mix(clean, None, bank, [0, 0], [0, 0], 0.0, out=torch.zeros(2, 63, device=DEV))
    with pytest.raises(L.AvvadError):
        ops.mix(clean.double(), None, bank, [0, 0], [0, 0], 0.0)


# ------------------------------------------------------------------ the chain and training
def _files(tmp_path):
    """two crops of the committed clean utterance and two seeded synthetic noise clips, as .npz utterances"""
    c = np.load(os.path.join(GOLDEN, "utt_sa1_clean.npz"))["samples"]
    rng = np.random.default_rng(5)
    clean, noise = [], []
    for k, (a, b) in enumerate(((2000, 22000), (9000, 23000))):
        clean.append(str(tmp_path / ("clean%d.npz" % k)))
        np.savez(clean[-1], samples=c[a:b], fs=np.array(16000))
    for k, n in enumerate((3000, 30000)):
        noise.append(str(tmp_path / ("noise%d.npz" % k)))
        np.savez(noise[-1], samples=(rng.standard_normal(n) * 2000).astype(np.int16), fs=np.array(16000))
    (tmp_path / "clean.txt").write_text("".join(p + "\n" for p in clean))
    (tmp_path / "noise.txt").write_text("".join(p + "\n" for p in noise))
    return clean, noise


def test_mix_step_is_wav_pair_step_on_the_mixture(tmp_path):
    from avvad import train as TR
    ops = _ops()
    dev = torch.device(DEV)
    clean_path = os.path.join(GOLDEN, "utt_sa1_clean.npz")
    _files(tmp_path)
    bank = TR.read_noise_bank(str(tmp_path / "noise.txt"), dev)
    assert bank.lengths == [3000, 30000]
    ds = TR.CleanWavs([clean_path, clean_path])
    batch = TR.CleanWavs.collate([ds[0], ds[1]])
    pairs = TR.WavPairs([(clean_path, clean_path)] * 2)
    pair_batch = TR.WavPairs.collate([pairs[0], pairs[1]])
    lens = [int(n) for n in batch[0]]
    for y_dim in (1, 513):
        labels = TR.labels_for_ydim(y_dim)
        mixer = TR.MixDraw(bank, (-5.0, 20.0), mix_seed=11, rank=0)
        frames, x, target, waves = TR.mix_step(batch, dev, labels, bank, mixer.seed(1), waves=True)
        want_frames, want_x, want_target = TR.wav_pair_step(pair_batch, dev, labels)
        assert torch.equal(frames, want_frames) and torch.equal(target, want_target)
        assert not torch.equal(x, want_x)                    # the features are the mixture's, not the clean file's
        clip, start, snr = mixer.seed(1)(lens)
        clean = ops.peak_normalize(batch[1].to(dev))
        noisy, noise_t, info = ops.mix(clean, lens, bank, clip, start, snr, return_noise=True, return_info=True)
        normed = ops.peak_normalize(noisy)
        assert torch.equal(x, ops.stft(normed, 1024, 256, mode=0, eps=1e-8, pad_at_end=True, fs=16e3))
        assert torch.equal(waves[0], normed) and torch.equal(waves[1], clean) and waves[2] == lens and torch.equal(waves[3], noise_t)
        assert torch.equal(info["peak"], ops.peak(noisy))
        realised = 10 * torch.log10(clean.double().pow(2).sum(1) / noise_t.double().pow(2).sum(1))
        assert (realised.cpu() - torch.tensor(snr, dtype=torch.float64)).abs().max() <= 1e-5
        # without the waves: the same three values
        again = TR.mix_step(batch, dev, labels, bank, mixer.seed(1))
        assert len(again) == 3 and torch.equal(again[1], x)


@pytest.mark.parametrize("objective,y_dim", [("bce", 1), ("si_sdr", 513)])
def test_training_on_mixtures_made_in_the_step(tmp_path, objective, y_dim):
    """DeepVAD_audio (one LSTM layer, hidden 32) on two clean crops and two noise clips, 2 epochs: finite losses in the log,
    and two runs with the same mix_seed end in the same parameter bits."""
    from avvad import train as TR
    from packages.models.Audio_Net import DeepVAD_audio
    _files(tmp_path)
    states = []
    for run in ("a", "b"):
        out = str(tmp_path / run)
        model = TR.train_main("audio", lambda: DeepVAD_audio(1, 32, y_dim), "mix", epochs=2, batch_size=2, lr=1e-3, out_dir=out,
                              clean_wavs=str(tmp_path / "clean.txt"), noise_wavs=str(tmp_path / "noise.txt"),
                              snr_db=(-5.0, 20.0), mix_seed=4, objective=objective, compute_stats=True)
        states.append({k: v.detach().clone() for k, v in model.state_dict().items()})
        log = open(os.path.join(out, "output_batch.log")).read()
        losses = [float(v) for v in re.findall(r"loss (\S+)", log)]
        assert len(re.findall(r"Epoch: +\d", log)) == 2 and len(losses) >= 4 and all(np.isfinite(losses)), log
        assert ("si-sdr" in log) == (objective == "si_sdr")
        assert "mixed utterances" in log and os.path.exists(os.path.join(out, "trainset_audio_mean.npy"))
        assert len(re.findall(r"valid loss (\S+)", log)) == 2
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k
