"""The streaming masked inverse STFT, the part that needs no GPU: the host-side bookkeeping of the samples a call emits
(``OlaClock``) against ``SampleClock``, the streamed overlap-add recurrence (tests/istft_stream_ref.py) against the
whole-utterance oracle (tests/istft_ref.py) for random splits of a stream, the descriptor checks and the refusals."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import istft_ref as R
import istft_stream_ref as SR

LENGTHS = (700, 3000, 5000, 5120)       # no frame at all; short; the end-pad branch of the frame count; no pad
N_FFT, HOP = 1024, 256


def _schedule(N, rng, lo, hi, n_fft=N_FFT, hop=HOP):
    """N samples in random packets, the last one final, through SampleClock and OlaClock -> [(frames, n_before, n_out)]"""
    from avvad.stream import OlaClock, SampleClock
    sc, oc = SampleClock(1, n_fft, hop), OlaClock(1, n_fft, hop)
    left, calls = N, []
    while True:
        n = min(left, rng.randint(lo, hi))
        left -= n
        fin = [0] if left == 0 else []
        frames = sc.advance([n], fin)[0]
        totals = {0: N} if fin else None
        before = (list(oc.emitted), list(oc.written), list(oc.ended))
        plan = oc.plan(frames, totals)
        assert (oc.emitted, oc.written, oc.ended) == before                       # plan changes nothing
        n_before, n_out = oc.advance(frames, totals)
        assert (n_before, n_out) == plan
        assert n_out[0] >= 0 and n_before[0] == sc.emitted[0] - frames[0] == before[0][0]
        if left > 0:
            assert n_out[0] == frames[0] * hop and oc.written[0] == oc.emitted[0] * hop
        assert oc.emitted == sc.emitted
        calls.append((frames[0], n_before[0], n_out[0]))
        if left == 0:
            assert oc.ended == [True] and oc.written == [N]
            return calls, sc, oc


@pytest.mark.parametrize("N", LENGTHS)
def test_ola_clock_counts_add_up_to_the_stream(N):
    from avvad import AvvadError, ops
    rng = random.Random(N)
    for lo, hi in ((1, 2000), (160, 160), (0, 300), (N, N)):
        calls, sc, oc = _schedule(N, rng, lo, hi)
        assert sum(c[2] for c in calls) == N and all(c[2] >= 0 for c in calls)
        assert sum(c[0] for c in calls) == max(ops.n_frames(N, N_FFT, HOP), 0) == sc.emitted[0]
        with pytest.raises(AvvadError, match="reset"):
            oc.plan([1])                                                          # a row that ended takes nothing
        with pytest.raises(AvvadError, match="reset"):
            oc.advance([0], {0: N})
        assert oc.plan([0]) == ([oc.emitted[0]], [0])                            # but it may idle
        oc.reset([0])
        assert oc.emitted == oc.written == [0] and oc.ended == [False]
        assert oc.advance([2]) == ([0], [2 * HOP])


def test_ola_clock_rows_and_refusals():
    from avvad import AvvadError
    from avvad.stream import OlaClock
    c = OlaClock(3, 64, 16)
    assert c.advance([2, 0, 5]) == ([0, 0, 0], [32, 0, 80])
    assert c.advance([1, 0, 0], [100, None, None]) == ([2, 0, 5], [68, 0, 0])     # row 0 ends with 100 samples
    assert c.advance([0, 0, 1], {1: 40}) == ([3, 0, 5], [0, 40, 16])              # row 1 never had a frame: 40 (zero) samples
    before = (list(c.emitted), list(c.written), list(c.ended))
    for frames, fin in (([0, 0, -1], None), ([0, 0], None), ([0, 0, 0], {3: 5}), ([0, 0, 0], [1, 2]), ([1, 0, 0], None),
                        ([0, 0, 0], {2: 50})):                                    # 50 < the 96 samples row 2 has written
        with pytest.raises(AvvadError):
            c.advance(frames, fin)
        assert (c.emitted, c.written, c.ended) == before
    c.reset([0, 1])
    assert c.emitted == [0, 0, 6] and c.written == [0, 0, 96] and c.ended == [False, False, False]
    for bad in ((0, 64, 16), (2, 64, 0), (2, 16, 64)):
        with pytest.raises(AvvadError):
            OlaClock(*bad)


@pytest.mark.parametrize("N", LENGTHS)
def test_streamed_overlap_add_equals_the_whole_utterance_oracle(N):
    """The float64 recurrence -- state in, frames, samples and state out -- over random splits of a stream of N samples
    against istft64 of all its frames, cropped or zero-filled to N: the same chain of additions, so the same float64
    values exactly; a stream that never completes a frame is N zeros."""
    from avvad import ops
    rng = random.Random(7 * N)
    T = max(ops.n_frames(N, N_FFT, HOP), 0)
    S = R.random_spectrum(np.random.default_rng(N), T, N_FFT) if T else np.zeros((0, N_FFT // 2 + 1), np.complex64)
    y64, num64, wss64 = R.istft64(S, N_FFT, HOP, length=N) if T else (np.zeros(N), np.zeros(N), np.zeros(N))
    for lo, hi in ((N, N), (1, 2000), (HOP, HOP), (0, 400)):
        calls = _schedule(N, rng, lo, hi)[0]
        y, num, wss, state = SR.stream(S, calls, N_FFT, HOP)
        assert y.shape == (N,)
        assert np.array_equal(num, num64) and np.array_equal(wss, wss64) and np.array_equal(y, y64), (N, lo, hi)
        assert not state.any()                                                    # all zero after the final flush
    if T == 0:
        assert not y.any()


def test_streamed_overlap_add_with_a_hop_that_does_not_divide_the_frame():
    n_fft, hop, T = 64, 48, 5
    S = R.random_spectrum(np.random.default_rng(3), T, n_fft)
    N = R.istft_length(T, n_fft, hop) - 7
    y64, num64, wss64 = R.istft64(S, n_fft, hop, length=N)
    for split in ([5], [1] * 5, [2, 0, 3], [0, 4, 1]):
        calls, t = [], 0
        for k, nf in enumerate(split):
            last = k == len(split) - 1
            calls.append((nf, t, N - t * hop if last else nf * hop))
            t += nf
        y, num, wss, state = SR.stream(S, calls, n_fft, hop)
        assert np.array_equal(num, num64) and np.array_equal(wss, wss64) and np.array_equal(y, y64), split
    # mid-stream the state is the partial sum of the samples later frames still cover, zero from n_fft - hop on
    Y = SR.frame_inverses(S, n_fft)
    _, _, st = SR.step(Y[:2], np.zeros(n_fft), 0, 2 * hop, n_fft, hop)
    assert np.array_equal(st[:n_fft - hop], Y[1][hop:]) and not st[n_fft - hop:].any()


def test_entry_points_validate_descriptors():
    from avvad import _lib as L
    h = L.lib()
    assert h.avvad_istft_stream_basis_bytes(1024) == 1024 * 1024 * 4 + 1024 * 8   # K = n_fft rows, hann^2 in double behind
    assert h.avvad_istft_stream_basis_bytes(2048) > 0                             # fits one 16-frame pass
    for bad in (0, 1000, 16, 4096):
        assert h.avvad_istft_stream_basis_bytes(bad) == 0
    assert h.avvad_istft_stream_basis(1024, None, None) == -1 and h.avvad_istft_stream_basis(1000, C.c_void_p(64), None) == -1
    good = L.IstftStreamDesc(2, 3, 1024, 256, 768, 5, 1)
    assert h.avvad_istft_stream_workspace(C.byref(good)) >= 2 * 3 * 1024 * 4
    flush = L.IstftStreamDesc(2, 0, 1024, 256, 700, 0, 0)                         # T == 0 with L > 0: a final flush
    assert h.avvad_istft_stream_workspace(C.byref(flush)) > 0
    one, two, ws = C.c_void_p(64), C.c_void_p(128), C.c_void_p(256)
    big = 1 << 30

    def call(d, spec=one, mask=one, si=one, so=two, basis=one, w=ws):
        return h.avvad_istft_stream(spec, mask, one, one, one, None, si, so, basis, one, C.byref(d), w, big, None)
    for bad in (L.IstftStreamDesc(0, 3, 1024, 256, 768, 0, 1), L.IstftStreamDesc(2, -1, 1024, 256, 768, 0, 1),
                L.IstftStreamDesc(2, 3, 1000, 256, 768, 0, 1), L.IstftStreamDesc(2, 3, 1024, 0, 768, 0, 1),
                L.IstftStreamDesc(2, 3, 1024, 2048, 768, 0, 1), L.IstftStreamDesc(2, 3, 1024, 256, -1, 0, 1),
                L.IstftStreamDesc(2, 3, 1024, 256, 768, 0, 4), L.IstftStreamDesc(2, 3, 4096, 256, 768, 0, 1)):
        assert h.avvad_istft_stream_workspace(C.byref(bad)) == 0 and call(bad) == -1
    assert call(good, si=one, so=one) == -1                                       # the state is read while it is written
    assert call(good, mask=None) == -1                                            # mask_mode 1 without a mask
    assert call(good, basis=C.c_void_p(68)) == -1 and call(good, w=C.c_void_p(260)) == -1      # off their 16 bytes
    assert call(good, spec=None) == -1
    assert h.avvad_istft_stream(one, one, one, one, one, None, one, two, one, one, C.byref(good), ws,
                                h.avvad_istft_stream_workspace(C.byref(good)) - 4, None) == -2
    sd = L.StftStreamDesc(2, 256, 1024, 256, 1, 2, 1e-8, 1e-8)
    args = [one, one, one, one, one, None, one, two, one, None, None, one]
    assert h.avvad_stft_stream_fwd_spec(*args, None, C.byref(sd), None) == -1                  # T > 0 needs spec
    assert h.avvad_stft_stream_fwd_spec(*args, C.c_void_p(68), C.byref(sd), None) == -1        # 8-byte aligned
    args[8] = C.c_void_p(68)
    assert h.avvad_stft_stream_fwd_spec(*args, one, C.byref(sd), None) == -1                   # the basis off its 16 bytes


def test_ops_refuse_cpu_tensors_and_bad_sizes():
    from avvad import AvvadError, ops
    from avvad.stream import OlaClock
    c = OlaClock(2, 1024, 256)
    with pytest.raises(AvvadError, match="GPU"):
        ops.istft_stream(torch.zeros(2, 1, 513, 2), [1, 1], c, torch.zeros(2, 1024), torch.zeros(8))
    with pytest.raises(AvvadError):
        ops.istft_stream_basis(1000, "cpu")
    with pytest.raises(AvvadError, match="GPU"):
        ops.istft_stream_basis(1024, "cpu")
    with pytest.raises(AvvadError):
        ops.istft_stream_state(0, 1024, "cpu")
    with pytest.raises(AvvadError):
        ops.istft_stream_state(2, 4096, "cpu")
    assert c.emitted == c.written == [0, 0]


def test_step_enhance_refusals_that_need_no_gpu():
    from avvad import AvvadError, stream
    from avvad import train as TR
    s = stream.Session.__new__(stream.Session)
    s.kind, s.enc, s.batch = "video", None, 2
    with pytest.raises(AvvadError, match="step_wave"):
        s.step_enhance(torch.zeros(2, 160))
    s.kind = "audio"
    s._frontend = dict(stats=None, eps=1e-8, n_fft=1024, hop=256)
    s.linear = torch.nn.Linear(4, 1)
    with pytest.raises(AvvadError, match="mask"):
        s.step_enhance(torch.zeros(2, 160))                                       # y_dim = 1 predicts no mask
    s.linear = torch.nn.Linear(4, 513)
    with pytest.raises(AvvadError, match="GPU"):
        s.step_enhance(torch.zeros(2, 160))
    with pytest.raises(ValueError, match="resynth_chunked"):
        TR.evaluate_main("audio", lambda: None, wav_list=[], resynth_chunked=True)
    with pytest.raises(ValueError, match="resynth_chunked"):
        TR.evaluate_main("audio", lambda: None, wav_list=[], resynth_chunked=True, chunk_samples=160)
