"""Streaming inference, the part that needs no GPU: the declared / bound / exported symbols, the host-side warm-up and
frame-count bookkeeping against a brute-force restatement, and the refusals."""
import os
import random
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("avvad_lstm_state_workspace", "avvad_lstm_layer_fwd_state", "avvad_wavenet_stream_state_bytes",
       "avvad_wavenet_stream_workspace", "avvad_wavenet_stream_fwd")


def test_stream_symbols_are_declared_bound_and_exported():
    from avvad import _lib as L
    h = L.lib()
    assert h.avvad_abi_version() == L.ABI_VERSION == 3            # added entry points change no signature
    header = open(os.path.join(ROOT, "include", "avvad.h")).read()
    declared = set(re.findall(r"\b(avvad_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(h, name), name
    assert "#define AVVAD_ABI_VERSION 3" in header


def test_stream_queries_validate_descriptors():
    import ctypes as C
    from avvad import _lib as L
    h = L.lib()
    dil = (C.c_int * 20)(*([2 ** i for i in range(10)] * 2))
    w0 = L.WavenetDesc(3, 256, 1, 32, 32, 256, 2, 1, 20, dil, 1, 0, 0)
    assert h.avvad_wavenet_stream_state_bytes(C.byref(w0)) == (4 + 1 + 32 * 2046) * 4 + 12     # rounded up to 16 bytes
    assert h.avvad_wavenet_stream_workspace(C.byref(w0)) > 0
    saved = L.WavenetDesc(3, 256, 1, 32, 32, 256, 2, 1, 20, dil, 1, 1, 0)
    assert h.avvad_wavenet_stream_state_bytes(C.byref(saved)) == 0      # inference only
    assert h.avvad_wavenet_stream_fwd(None, None, None, None, None, 256, None, 0, C.byref(w0), None, 0, None) == -1
    assert h.avvad_lstm_state_workspace(C.byref(L.LstmDesc(3, 5, 513, 1024, None, 0))) > 0
    assert h.avvad_lstm_state_workspace(C.byref(L.LstmDesc(3, 5, 513, 1024, None, 1))) == 0
    assert h.avvad_lstm_state_workspace(C.byref(L.LstmDesc(0, 5, 513, 1024, None, 0))) == 0
    assert h.avvad_lstm_layer_fwd_state(*([None] * 10), C.byref(L.LstmDesc(3, 5, 513, 1024, None, 0)), None, 0, None) == -1


class _BruteRow:
    """One row restated sample by sample: sample i since the reset gives an output column iff i >= RF-1; a frame is k
    output columns; a call is legal iff it ends on a frame boundary (or before the first column)."""

    def __init__(self, rf, k):
        self.rf, self.k, self.seen = rf, k, 0

    def cols(self, seen):
        return max(0, seen - (self.rf - 1))

    def feed(self, n):
        before, after = self.cols(self.seen), self.cols(self.seen + n)
        if after % self.k:
            return None
        self.seen += n
        return after // self.k - before // self.k


@pytest.mark.parametrize("rf,k,seed", [(2048, 256, 0), (17, 71, 1), (1, 4, 2), (6, 1, 3), (2048, 256, 4)])
def test_frame_clock_matches_brute_force(rf, k, seed):
    from avvad import AvvadError
    from avvad.stream import FrameClock
    rng = random.Random(seed)
    B = 4
    clock = FrameClock(B, rf, k)
    rows = [_BruteRow(rf, k) for _ in range(B)]
    refused = partial = 0
    for it in range(400):
        if rng.random() < 0.1:                                    # reset a subset of the rows
            sub = [b for b in range(B) if rng.random() < 0.5]
            clock.reset(sub)
            for b in sub:
                rows[b] = _BruteRow(rf, k)
        n = []
        for b in range(B):
            mode = rng.random()
            left = clock.skip[b]
            if mode < 0.2:
                n.append(0)
            elif mode < 0.45 and left > 0:                        # a partial warm-up chunk
                n.append(rng.randint(1, left))
                partial += 1
            elif mode < 0.9:
                n.append(left + k * rng.randint(1, 3))
            else:
                n.append(left + k * rng.randint(0, 2) + rng.randint(1, k) )   # off the grid unless k divides it
        want = [r.cols(r.seen + nb) % k == 0 for r, nb in zip(rows, n)]
        if not all(want):
            before = list(clock.skip)
            with pytest.raises(AvvadError):
                clock.advance(n)
            assert clock.skip == before                           # a refused call changes nothing
            refused += 1
            continue
        frames, used = clock.advance(n)
        assert used == [max(0, rf - 1 - r.seen) for r in rows]
        assert frames == [r.feed(nb) for r, nb in zip(rows, n)]
        assert clock.skip == [max(0, rf - 1 - r.seen) for r in rows]
    assert refused > 0 or k == 1
    assert partial > 0 or rf == 1


def test_frame_clock_first_frame_needs_the_whole_receptive_field():
    from avvad import AvvadError
    from avvad.stream import FrameClock
    c = FrameClock(2, 2048, 256)
    assert c.advance([2047, 1000]) == ([0, 0], [2047, 2047])
    assert c.skip == [0, 1047]
    assert c.plan([512, 1047 + 256]) == [2, 1]
    with pytest.raises(AvvadError):
        c.plan([255, 0])
    with pytest.raises(AvvadError):
        c.plan([256, 1048])
    with pytest.raises(AvvadError):
        c.plan([256])
    c.reset([0])
    assert c.skip == [2047, 1047]


def test_open_refuses_what_cannot_be_streamed():
    from avvad import AvvadError, stream
    from packages.models.Audio_Net import DeepVAD_audio
    from packages.models.AV_Net import DeepVAD_AV
    with pytest.raises(AvvadError, match="eval"):
        stream.open(DeepVAD_audio(1, 8, 1).train(), 2)
    with pytest.raises(AvvadError, match="L2 norm"):
        stream.open(DeepVAD_AV(1, 8, 1, use_mcb=True).eval(), 2)
    with pytest.raises(AvvadError, match="GPU"):
        stream.open(DeepVAD_audio(1, 8, 1).eval(), 2)             # a model on the CPU (or no GPU at all)
    with pytest.raises(AvvadError):
        stream.open(torch.nn.Linear(2, 2).eval(), 1)


def test_ops_refuse_cpu_tensors():
    from avvad import AvvadError, ops
    from packages.models.wavenet_autoencoder import wavenet_autoencoder
    lstm = torch.nn.LSTM(4, 8, 1)
    with pytest.raises(AvvadError, match="GPU"):
        ops.lstm_stack_state(torch.zeros(2, 3, 4), [3, 3], lstm)
    enc = wavenet_autoencoder(2, 1, [1, 2], 4, 4, 8, 1, True)
    with pytest.raises(AvvadError, match="GPU"):
        ops.wavenet_stream(torch.zeros(2, 1, 16), [16, 16], [3, 3], enc, torch.zeros(2, 24), 4, 3)
