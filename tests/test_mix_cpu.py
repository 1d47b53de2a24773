"""The SNR mix (csrc/mix.hip), the part that needs no GPU: the declared / bound / exported symbols, the chunk constant and
the workspace query, the refusals of the C ABI with never-dereferenced pointers, the host logic (``NoiseBank``, the
seeded draws, the argument errors of ``train_main`` and ``check_objective``), and the assertions of tests/mix_ref.py
themselves: a float32 numpy stand-in passes them and each of nine built-in mistakes is rejected; the 70-row case, and the
mistake of a gain kernel that stops after its first 64 rows, which that case alone rejects."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mix_ref
from conftest import ROOT

NEW = ("avvad_mix_workspace", "avvad_mix")


def test_mix_symbols_are_declared_bound_and_exported():
    from avvad import _lib as L, ops
    h = L.lib()
    assert h.avvad_abi_version() == L.ABI_VERSION == 3            # added entry points change no signature
    header = open(os.path.join(ROOT, "include", "avvad.h")).read()
    assert int(re.search(r"#define AVVAD_ABI_VERSION (\d+)", header).group(1)) == 3
    declared = set(re.findall(r"\b(avvad_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(h, name), name
    build = open(os.path.join(ROOT, "audio-visual-vad_amd", "csrc", "build.sh")).read()
    assert re.search(r'SRCS="[^"]*\bmix\b[^"]*"', build)
    chunk = int(re.search(r"#define AVVAD_MIX_CHUNK (\d+)", header).group(1))
    assert chunk == L.MIX_CHUNK == ops.MIX_CHUNK == mix_ref.CHUNK == 4096        # (the case list names 4095 .. 4097)


def test_workspace_query():
    from avvad import _lib as L
    h = L.lib()
    chunk = L.MIX_CHUNK
    # one (Es, En) pair of doubles per (row, chunk) rounded up to 256 bytes, then one float per row rounded up likewise
    assert h.avvad_mix_workspace(1, 1) == h.avvad_mix_workspace(1, 16 * chunk) == 512
    assert h.avvad_mix_workspace(1, 16 * chunk + 1) == 512 + 256
    assert h.avvad_mix_workspace(64, chunk) == 64 * 16 + 256 and h.avvad_mix_workspace(65, chunk) == 1280 + 512
    assert h.avvad_mix_workspace(16, 80000) == 16 * -(-80000 // chunk) * 16 + 256
    assert h.avvad_mix_workspace(0, 100) == h.avvad_mix_workspace(1, 0) == h.avvad_mix_workspace(65536, 1) == 0


def test_refusals_need_no_gpu():
    from avvad import _lib as L, ops
    h = L.lib()
    p = lambda v: C.c_void_p(v)                              # noqa: E731  (never dereferenced: every call is refused first)
    L_ = 10
    #      clean     ld  n_samples bank      n_bank clip_off  clip_len  K  clip      start     ratio
    ok = [p(0x1000), L_, None, p(0x2000), 100, p(0x3000), p(0x4000), 2, p(0x5000), p(0x6000), p(0x7000),
          # noisy   ld  noise_out  ld  gain       energies   peak       B  L   ws          bytes stream
          p(0x8000), L_, p(0x9000), L_, p(0xa000), p(0xb000), p(0xc000), 1, L_, p(0x10000), 512, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return h.avvad_mix(*a)
    for i in (0, 3, 5, 6, 8, 9, 10, 11, 20):                 # a NULL where a pointer is required
        assert call(**{"a%d" % i: None}) == -1, i
    assert call(a1=L_ - 1) == call(a12=L_ - 1) == call(a14=L_ - 1) == -1          # a pitch below L
    assert call(a20=p(0x10004)) == call(a20=p(0x10008)) == -1                      # ws off its 16 bytes
    assert call(a10=p(0x7004)) == call(a16=p(0xb004)) == call(a5=p(0x3004)) == -1  # ratio / energies / clip_off off their 8
    assert call(a7=0) == call(a7=-1) == call(a4=0) == -1                           # K < 1, an empty bank
    assert call(a11=p(0x1000)) == call(a13=p(0x1000)) == call(a13=p(0x8000)) == -1   # noisy == clean, noise_out == either
    assert call(a18=0) == call(a18=65536) == call(a19=0) == -1
    assert call(a21=511) == -2                                                     # one byte short
    assert call(a13=None, a14=0, a21=511) == -2              # (without noise_out its pitch does not count)
    with pytest.raises(L.AvvadError, match="GPU"):
        ops.mix(torch.zeros(2, 8), None, ops.NoiseBank([torch.ones(3)], "cpu"), [0, 0], [0, 0], [0.0, 0.0])


def test_noise_bank_layout():
    from avvad import _lib as L, ops
    bank = ops.NoiseBank([torch.arange(3.0), np.array([7.0, 8.0], dtype=np.float64), torch.full((5,), 2.0)], "cpu")
    assert bank.K == len(bank) == 3 and bank.offsets == [0, 3, 5] and bank.lengths == [3, 2, 5]
    assert bank.data.dtype == torch.float32 and bank.data.tolist() == [0, 1, 2, 7, 8, 2, 2, 2, 2, 2]
    assert bank.clip_off.dtype == torch.int64 and bank.clip_off.tolist() == bank.offsets
    assert bank.clip_len.dtype == torch.int32 and bank.clip_len.tolist() == bank.lengths
    for bad in ([], [torch.zeros(0)], [torch.zeros(2, 2)]):
        with pytest.raises(L.AvvadError):
            ops.NoiseBank(bad, "cpu")
    assert ops.mix_ratio(10.0) == 10.0 and ops.mix_ratio(0.0) == 1.0 and ops.mix_ratio(-20.0) == float(np.power(10, np.float64(-2.0)))


def test_draws_are_seeded_by_seed_epoch_and_rank():
    from avvad import ops, train
    bank = ops.NoiseBank([torch.ones(n) for n in (1, 300, 5000, 80000)], "cpu")
    lengths = [100] * 64
    draw = lambda seed, epoch, rank: train.draw_mix(train.mix_generator(seed, epoch, rank), lengths, bank, (-5.0, 20.0))   # noqa: E731
    a = draw(0, 1, 0)
    assert a == draw(0, 1, 0)
    for other in (draw(0, 2, 0), draw(0, 1, 1), draw(1, 1, 0), draw(0, "valid", 0)):
        assert other != a and other[0] != a[0] and other[2] != a[2]
    assert draw(0, "valid", 0) == draw(0, "valid", 0)
    clip, start, snr = a
    assert len(clip) == len(start) == len(snr) == 64 and set(clip) == {0, 1, 2, 3}
    assert all(0 <= s < bank.lengths[k] for k, s in zip(clip, start)) and all(-5.0 <= v <= 20.0 for v in snr)
    assert max(snr) - min(snr) > 12.5                         # uniform over the range, not a few fixed values
    assert train.draw_mix(train.mix_generator(0, 1, 0), [1, 2], bank, 7.5)[2] == [7.5, 7.5]
    # the pass of a MixDraw: consecutive batches continue one stream, seed() restarts it
    mixer = train.MixDraw(bank, (-5.0, 20.0), mix_seed=3, rank=1)
    with pytest.raises(RuntimeError):
        mixer([1])
    first, second = mixer.seed(1)([1] * 8), mixer([1] * 8)
    assert first != second and mixer.seed(1)([1] * 8) == first and mixer.seed(2)([1] * 8) != first
    for bad in ((5.0, -5.0), (0.0, float("inf")), (float("nan"), 1.0), "loud"):
        with pytest.raises(ValueError):
            train.draw_mix(train.mix_generator(0, 1, 0), [1], bank, bad)


def test_argument_errors_of_train_main_and_check_objective(tmp_path):
    from avvad import train
    train.check_objective("si_sdr", "audio", False, None, 513, clean_wavs=["a.wav"])
    train.check_objective("bce", "audio", False, None, 1, clean_wavs=["a.wav"])
    with pytest.raises(ValueError, match="si_sdr"):
        train.check_objective("si_sdr", "audio", False, None, 513)
    with pytest.raises(ValueError, match="513"):
        train.check_objective("si_sdr", "audio", False, None, 1, clean_wavs=["a.wav"])
    with pytest.raises(ValueError, match="si_sdr"):
        train.check_objective("si_sdr", "video", False, None, 513, clean_wavs=["a.wav"])
    never = lambda: pytest.fail("the model must not be built before the arguments are checked")   # noqa: E731
    kw = dict(out_dir=str(tmp_path))
    with pytest.raises(ValueError, match="go together"):
        train.train_main("audio", never, "m", clean_wavs=["a.npz"], **kw)
    with pytest.raises(ValueError, match="go together"):
        train.train_main("audio", never, "m", noise_wavs=["n.npz"], **kw)
    with pytest.raises(ValueError, match="one data source"):
        train.train_main("audio", never, "m", clean_wavs=["a.npz"], noise_wavs=["n.npz"], wav_pairs=[("a", "b")], **kw)
    with pytest.raises(ValueError, match="one data source"):
        train.train_main("audio", never, "m", clean_wavs=["a.npz"], noise_wavs=["n.npz"], av_files=[("a", "b", "c")], **kw)
    with pytest.raises(ValueError, match="audio network"):
        train.train_main("video", never, "m", clean_wavs=["a.npz"], noise_wavs=["n.npz"], **kw)
    with pytest.raises(ValueError, match="audio network"):
        train.train_main("audio", never, "m", waveform=True, clean_wavs=["a.npz"], noise_wavs=["n.npz"], **kw)
    with pytest.raises(ValueError, match="snr_db"):
        train.train_main("audio", never, "m", clean_wavs=["a.npz"], noise_wavs=["n.npz"], snr_db=(20.0, -5.0), **kw)
    # the lists
    listing = tmp_path / "clean.txt"
    listing.write_text("# clean utterances\n a.npz \n\nb.npz  # the second\n")
    assert train.CleanWavs(str(listing)).paths == ["a.npz", "b.npz"] and train.CleanWavs(["c.npz"]).paths == ["c.npz"]
    lens, clean = train.CleanWavs.collate([(torch.ones(3), 3), (torch.ones(5), 5)])
    assert lens.tolist() == [3, 5] and clean.shape == (2, 5) and clean[0].tolist() == [1, 1, 1, 0, 0]
    np.savez(tmp_path / "n8k.npz", samples=np.zeros(10, np.int16), fs=8000)
    with pytest.raises(ValueError, match="16 kHz"):
        train.read_noise_bank([str(tmp_path / "n8k.npz")], "cpu")
    np.savez(tmp_path / "n16k.npz", samples=np.arange(10, dtype=np.int16), fs=16000)
    bank = train.read_noise_bank([str(tmp_path / "n16k.npz")] * 2, "cpu")
    assert bank.lengths == [10, 10] and bank.data[11].item() == 1.0 / 32768.0


@pytest.mark.parametrize("name", ["ragged", "wide"])
def test_float32_standin_passes_the_assertions(name):
    got = mix_ref.check_named(mix_ref.standin, name)
    case = mix_ref.ragged_case() if name == "ragged" else mix_ref.wide_case()
    assert case["clean"].shape[0] == (12 if name == "ragged" else 33) and case["L"] > max(case["lengths"])
    for b in mix_ref.DEGENERATE:
        assert got["gain"][b] == 0.0
    assert (got["gain"][[b for b in range(12) if b not in mix_ref.DEGENERATE]] > 0).all()


def test_wide70_puts_live_rows_behind_the_first_64():
    case = mix_ref.wide70_case()
    assert case["clean"].shape[0] == len(case["lengths"]) == 70 and case["L"] > max(case["lengths"])
    assert [case["lengths"][b] for b in range(64, 70)] == [r[0] for r in mix_ref.ROWS[4:10]]
    assert [(case["clip"][b], case["start"][b]) for b in range(64, 70)] == [r[1:3] for r in mix_ref.ROWS[4:10]]
    assert not any(b % len(mix_ref.ROWS) in mix_ref.DEGENERATE for b in range(64, 70))
    assert {case["snr_db"][b] for b in range(64, 70)} == {-20.0, 0.0, 7.5, 40.0}
    got = mix_ref.check_named(mix_ref.standin, "wide70")
    for b in range(70):
        assert (got["gain"][b] == 0.0) == (b % len(mix_ref.ROWS) in mix_ref.DEGENERATE), b
    assert (got["energies"][64:] > 0).all()


@pytest.mark.parametrize("mutant", mix_ref.LOOP_MUTANTS)
def test_the_loop_mutant_is_rejected_on_wide70_alone(mutant):
    broken = lambda case: mix_ref.standin(case, mutant)      # noqa: E731
    with pytest.raises(AssertionError):
        mix_ref.check_named(broken, "wide70")
    for name in ("ragged", "wide"):                          # at most 33 rows: the old cases could not see it
        got, want = mix_ref.check_named(broken, name), mix_ref.standin(mix_ref.NAMED[name]())
        assert all(np.array_equal(got[k], want[k]) for k in want), name


def test_a_row_alone_is_a_case_of_its_own():
    case = mix_ref.ragged_case()
    whole = mix_ref.standin(case)
    for b in (4, 7):
        one = mix_ref.check(mix_ref.standin, mix_ref.single_row(case, b))
        assert np.array_equal(one["noisy"][0], whole["noisy"][b]) and one["gain"][0] == whole["gain"][b]


@pytest.mark.parametrize("mutant", mix_ref.MUTANTS)
def test_each_mutant_is_rejected(mutant):
    with pytest.raises(AssertionError):
        mix_ref.check_named(lambda case: mix_ref.standin(case, mutant), "ragged")
