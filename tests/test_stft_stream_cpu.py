"""The streaming STFT front-end, the part that needs no GPU: the declared / bound / exported symbols, the host-side
sample bookkeeping against a brute-force count and the reference's frame count, resets and the refusals."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("avvad_stft_stream_basis_bytes", "avvad_stft_stream_basis", "avvad_stft_stream_fwd", "avvad_abs_max")


def test_stft_stream_symbols_are_declared_bound_and_exported():
    from avvad import _lib as L
    h = L.lib()
    assert h.avvad_abi_version() == L.ABI_VERSION == 3            # added entry points change no signature
    header = open(os.path.join(ROOT, "include", "avvad.h")).read()
    declared = set(re.findall(r"\b(avvad_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(h, name), name
    build = open(os.path.join(ROOT, "audio-visual-vad_amd", "csrc", "build.sh")).read()
    assert build.count("stft_stream") == 2                        # compiled and linked


def test_stft_stream_entry_points_validate_descriptors():
    from avvad import _lib as L
    h = L.lib()
    assert h.avvad_stft_stream_basis_bytes(1024) == 33 * 2 * 16 * 1024 * 4     # 33 blocks of 16 bins, re and im apart
    assert h.avvad_stft_stream_basis_bytes(512) == 17 * 2 * 16 * 512 * 4
    assert h.avvad_stft_stream_basis_bytes(1000) == 0 and h.avvad_stft_stream_basis_bytes(0) == 0    # n_fft % 32
    assert h.avvad_stft_stream_basis(1000, None, None) == -1
    assert h.avvad_stft_stream_basis(1024, None, None) == -1
    good = L.StftStreamDesc(2, 256, 1024, 256, 1, 2, 1e-8, 1e-8)
    assert h.avvad_stft_stream_fwd(*([None] * 12), C.byref(good), None) == -1
    one = C.c_void_p(64)                                          # non-NULL, never dereferenced: the descriptor is refused first
    two = C.c_void_p(128)
    for bad in (L.StftStreamDesc(0, 256, 1024, 256, 1, 0, 1e-8, 1e-8), L.StftStreamDesc(2, 0, 1024, 256, 1, 0, 1e-8, 1e-8),
                L.StftStreamDesc(2, 256, 1000, 256, 1, 0, 1e-8, 1e-8), L.StftStreamDesc(2, 256, 1024, 0, 1, 0, 1e-8, 1e-8),
                L.StftStreamDesc(2, 256, 1024, 2048, 1, 0, 1e-8, 1e-8), L.StftStreamDesc(2, 256, 1024, 256, -1, 0, 1e-8, 1e-8),
                L.StftStreamDesc(2, 256, 4096, 256, 1, 0, 1e-8, 1e-8)):                   # a pass of frames must fit LDS
        assert h.avvad_stft_stream_fwd(one, one, one, one, one, None, one, two, one, None, None, one, C.byref(bad), None) == -1
    # the state is read while it is written: in and out must differ; mean and std come together
    assert h.avvad_stft_stream_fwd(one, one, one, one, one, None, one, one, one, None, None, one, C.byref(good), None) == -1
    assert h.avvad_stft_stream_fwd(one, one, one, one, one, None, one, two, one, one, None, one, C.byref(good), None) == -1
    assert h.avvad_abs_max(None, None, 1, 10, None) == -1


def _brute_frames(N, n_fft, hop):
    """frames whose last sample has arrived, counted one by one"""
    t = 0
    while t * hop + n_fft <= N:
        t += 1
    return t


def _feed(clock, L, rng, lo, hi, row=0, rows=1):
    """L samples into ``row`` in random packets, the last one final -> (frames, calls)"""
    left, total, calls = L, 0, 0
    while True:
        n = min(left, rng.randint(lo, hi))
        left -= n
        vec = [0] * rows
        vec[row] = n
        fin = [row] if left == 0 else []
        before = (list(clock.total), list(clock.emitted), list(clock.pending))
        plan = clock.plan(vec, fin)
        assert (list(clock.total), list(clock.emitted), list(clock.pending)) == before          # plan changes nothing
        frames, used, pad = clock.advance(vec, fin)
        assert frames == plan and used == before[2]
        assert all(p in (0, 1) for p in pad) and (left == 0 or pad[row] == 0)
        assert 0 <= clock.pending[row] < clock.n_fft
        if left > 0:
            assert clock.emitted[row] == _brute_frames(clock.total[row], clock.n_fft, clock.hop)
            assert clock.pending[row] == clock.total[row] - clock.emitted[row] * clock.hop
        total += frames[row]
        calls += 1
        if left == 0:
            return total, calls


def test_sample_clock_matches_the_reference_frame_count_for_every_length():
    """Every L in 1..6000 (the lengths below n_fft, 769..1023 where only the padded frame exists, whole-hop lengths with
    and without the float test's pad) in random packets ending with ``final``: the frames add up to ops.n_frames(L)."""
    from avvad import ops
    from avvad.stream import SampleClock
    rng = random.Random(11)
    owed = set()
    for L in range(1, 6001):
        c = SampleClock(1, 1024, 256)
        total, _ = _feed(c, L, rng, 0, 700)
        want = max(ops.n_frames(L, 1024, 256), 0)
        assert total == want, (L, total, want)
        owed.add(want - _brute_frames(L, 1024, 256))
    assert owed == {0, 1}                                         # the final call owes nothing or the one padded frame
    assert max(ops.n_frames(1000, 1024, 256), 0) == 1 and _brute_frames(1000, 1024, 256) == 0


@pytest.mark.parametrize("n_fft,hop,lo,hi,seed", [(1024, 256, 1, 2000, 0), (1024, 256, 160, 160, 1), (1024, 256, 1, 3, 2),
                                                  (512, 128, 1, 900, 3)])
def test_sample_clock_on_the_golden_utterance(n_fft, hop, lo, hi, seed):
    from avvad import ops
    from avvad.stream import SampleClock
    L = int(np.load(os.path.join(GOLDEN, "utt_sa1.npz"))["samples"].shape[0])
    assert L == 48100
    c = SampleClock(3, n_fft, hop)
    total, calls = _feed(c, L, random.Random(seed), lo, hi, row=1, rows=3)
    assert total == max(ops.n_frames(L, n_fft, hop), 0) and calls >= L // hi
    assert c.total == [0, L, 0] and c.emitted[0] == c.emitted[2] == 0         # the idle rows stay where they were


def test_sample_clock_resets_subsets_of_rows():
    from avvad import AvvadError
    from avvad.stream import SampleClock
    c = SampleClock(4, 1024, 256)
    assert c.advance([1023, 1024, 1279, 1280]) == ([0, 1, 1, 2], [0, 0, 0, 0], [0, 0, 0, 0])
    assert c.pending == [1023, 768, 1023, 768] and c.emitted == [0, 1, 1, 2]
    assert c.plan([1, 0, 1, 256]) == [1, 0, 1, 1]
    c.reset([0, 3])
    assert c.total == [0, 1024, 1279, 0] and c.pending == [0, 768, 1023, 0] and c.emitted == [0, 1, 1, 0]
    assert c.plan([1, 0, 1, 256]) == [0, 0, 1, 0]
    frames, used, pad = c.advance([0, 100, 0, 900], final=[1, 3])             # 1124 and 900 samples end: one padded frame each
    assert frames == [0, 1, 0, 1] and used == [0, 768, 1023, 0] and pad == [0, 1, 0, 1]
    with pytest.raises(AvvadError, match="reset"):
        c.plan([0, 1, 0, 0])                                      # samples after final
    with pytest.raises(AvvadError, match="reset"):
        c.plan([0, 0, 0, 0], final=[3])                           # a second end
    assert c.plan([5, 0, 5, 0]) == [0, 0, 1, 0]                   # an ended row may idle
    c.reset([1])
    assert c.plan([0, 1024, 0, 0]) == [0, 1, 0, 0]
    c.reset()
    assert c.total == c.emitted == c.pending == [0, 0, 0, 0] and c.ended == [False] * 4


def test_sample_clock_refusals_change_nothing():
    from avvad import AvvadError
    from avvad.stream import SampleClock
    c = SampleClock(2, 1024, 256)
    c.advance([500, 2000])
    before = (list(c.total), list(c.emitted), list(c.pending), list(c.ended))
    for n, fin in (([-1, 0], ()), ([0, -5], ()), ([1], ()), ([1, 2, 3], ()), ([1, 1], [2]), ([1, 1], [-1])):
        with pytest.raises(AvvadError):
            c.advance(n, final=fin)
        with pytest.raises(AvvadError):
            c.plan(n, final=fin)
        assert (c.total, c.emitted, c.pending, c.ended) == before
    for bad in ((0, 1024, 256), (2, 1024, 0), (2, 256, 1024)):
        with pytest.raises(AvvadError):
            SampleClock(*bad)


def test_ops_refuse_cpu_tensors_and_bad_sizes():
    from avvad import AvvadError, ops
    from avvad.stream import SampleClock
    c = SampleClock(2, 1024, 256)
    with pytest.raises(AvvadError, match="GPU"):
        ops.stft_stream(torch.zeros(2, 160), None, c, torch.zeros(2, 1024), torch.zeros(8))
    with pytest.raises(AvvadError, match="GPU"):
        ops.peak(torch.zeros(2, 160))
    with pytest.raises(AvvadError):
        ops.stft_stream_basis(1000, "cpu")
    with pytest.raises(AvvadError):
        ops.stft_stream_state(0, 1024, "cpu")
    with pytest.raises(AvvadError):
        ops.stft_stream_state(2, 4096, "cpu")
    assert c.total == [0, 0]


def test_step_wave_refuses_models_without_the_spectrogram_front_end():
    """A session cannot be opened without a GPU, so the refusals that come before any GPU work are checked on a bare
    object: the video model, a model with the encoder, CPU tensors, a wave that is not float32."""
    from avvad import AvvadError, stream
    s = stream.Session.__new__(stream.Session)
    s.kind, s.enc, s.batch = "video", None, 2
    with pytest.raises(AvvadError, match="step_wave"):
        s.step_wave(torch.zeros(2, 160))
    with pytest.raises(AvvadError, match="step_wave"):
        s.set_frontend()
    s.kind, s.enc = "audio", object()
    with pytest.raises(AvvadError, match="encoder"):
        s.step_wave(torch.zeros(2, 160))
    s.enc = None
    with pytest.raises(AvvadError, match="GPU"):
        s.step_wave(torch.zeros(2, 160))
    with pytest.raises(AvvadError, match="GPU"):
        s.step_wave(torch.zeros(2, 160, dtype=torch.float64))


def test_evaluators_refuse_two_kinds_of_chunking():
    from avvad import train as TR
    with pytest.raises(ValueError, match="exclude"):
        TR.process_utt(None, torch.zeros(2000), chunk_frames=4, chunk_samples=160)
    with pytest.raises(ValueError, match="exclude"):
        TR.evaluate_main("audio", lambda: None, wav_list=[], chunk_frames=4, chunk_samples=160)
    with pytest.raises(ValueError, match="chunk_samples"):
        TR.evaluate_main("audio", lambda: None, chunk_samples=160)            # the synthetic source has no waveform
    with pytest.raises(ValueError, match="chunk_samples"):
        TR.evaluate_main("video", lambda: None, av_files=[], chunk_samples=160)
