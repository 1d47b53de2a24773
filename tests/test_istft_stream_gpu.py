"""The streaming masked inverse STFT on the GPU (csrc/istft_stream.hip, ``ops.istft_stream``, ``Session.step_enhance``).

Values go against the float64 oracle of tests/istft_ref.py by that module's yardstick, the one of tests/test_istft_gpu.py:
``E = max_s |y[s] wss64[s] - num64[s]| <= 8 E_cpu32``, ``E_cpu32`` the same measure of the float32 CPU evaluation of the GEMM
form on the same (masked) spectrum.  Exact properties -- any split of a stream into calls, idle rows, rows reset beside
rows that go on, mask mode 3 against the 0/1 mask, zeros behind a row's count -- are compared bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

import istft_ref as R
from conftest import GOLDEN, load_golden

from test_istft_gpu import _check_row, _covered, _logits
from test_istft_gpu import _report as _ireport

pytestmark = pytest.mark.gpu
T_ = torch.from_numpy
DEV = "cuda:0"
NAN = float("nan")


def _split(T, k):
    """T frames over k calls, as evenly as they go (the first calls take the larger share)"""
    return [len(c) for c in np.array_split(np.arange(T), k)]


def _run(rows, n_fft, hop, schedule, totals=None, masks=None, mode=None, scale=None, state=None, clock=None, resets=None, end=True):
    """Rows of complex (T_b, F) spectra through ops.istft_stream: ``schedule[call][b]`` frames of row b per call.  Row b
    ends (``final_samples`` = ``totals[b]``, default its natural length) with the last call that gives it a frame, a row
    without frames with the last call.  The padding frames of spec and mask hold NaN.  ``resets``: {call: (rows,
    new spectra)} -- before that call the rows are reset and start over on the new spectra.  ``end=False``: no row ends.
    -> (per-row samples, the last state, samples per call and row)"""
    from avvad import ops
    from avvad.stream import OlaClock
    B, F = len(rows), n_fft // 2 + 1
    rows = list(rows)
    basis = ops.istft_stream_basis(n_fft, DEV)
    clock = OlaClock(B, n_fft, hop) if clock is None else clock
    state = ops.istft_stream_state(B, n_fft, DEV) if state is None else state
    spare = torch.full_like(state, NAN)
    if totals is None:
        totals = [R.istft_length(S.shape[0], n_fft, hop) for S in rows]
    last = [max([c for c, counts in enumerate(schedule) if counts[b] > 0] + ([len(schedule) - 1] if rows[b].shape[0] == 0 else []))
            if rows[b] is not None else -1 for b in range(B)]
    pos, outs, per_call = [0] * B, [[] for _ in range(B)], []
    for c, counts in enumerate(schedule):
        if resets and c in resets:
            which, new = resets[c]
            clock.reset(which)
            for b, S in zip(which, new):
                state[b].zero_()
                rows[b], pos[b], outs[b] = S, 0, []
        tmax = max(counts)
        spec = np.full((B, tmax, F, 2), NAN, dtype=np.float32)
        m = None if masks is None else np.full((B, tmax, F), NAN, dtype=np.float32)
        for b, k in enumerate(counts):
            if k:
                S = rows[b][pos[b]:pos[b] + k]
                spec[b, :k, :, 0], spec[b, :k, :, 1] = S.real, S.imag
                if m is not None:
                    m[b, :k] = masks[b][pos[b]:pos[b] + k]
        fin = {b: totals[b] for b in range(B) if end and last[b] == c}
        y, n_out = ops.istft_stream(T_(spec).to(DEV), counts, clock, state, basis, None if m is None or tmax == 0 else T_(m).to(DEV),
                                    mode, scale, fin, spare)
        state, spare = spare, state
        assert y.shape == (B, max(n_out)) and y.dtype == torch.float32
        for b, k in enumerate(counts):
            assert clock.written[b] == totals[b] if b in fin else n_out[b] == k * hop
            assert torch.count_nonzero(y[b, n_out[b]:]).item() == 0 and not torch.signbit(y[b, n_out[b]:]).any()
            outs[b].append(y[b, :n_out[b]])
            pos[b] += k
        per_call.append(n_out)
    return [torch.cat(o) if o else torch.zeros(0, device=DEV) for o in outs], state, per_call


def _spectra(n_fft, frames, seed):
    rng = np.random.default_rng(seed)
    return [R.random_spectrum(rng, T, n_fft) if T else np.zeros((0, n_fft // 2 + 1), np.complex64) for T in frames]


PARITY = [(64, 16, [9, 4, 1], 3), (96, 24, [7, 2], 2), (64, 48, [5, 3], 4), (1024, 256, [37, 5], 0), (64, 16, [1 + b % 2 for b in range(70)], 2)]


@pytest.mark.parametrize("n_fft,hop,frames,calls", PARITY, ids=lambda v: str(v) if not isinstance(v, list) else "%dx%d" % (len(v), max(v)))
def test_parity_with_the_oracle(n_fft, hop, frames, calls):
    """Random spectra streamed in 2 to 4 calls against istft64 of all their frames: K = 64 holds 4 sample groups for the 8
    waves; an FFT length that is no power of two; a hop that does not divide it; ONE call of 42 frames across the pass
    boundary of 32 (its rows end in a second call without frames: T == 0, L > 0); 70 rows, more than one 64-lane scan.
    Padding frames hold NaN."""
    rows = _spectra(n_fft, frames, seed=n_fft + hop + len(frames))
    B = len(frames)
    if calls:
        per_row = [_split(T, calls) for T in frames]
        schedule = [[per_row[b][c] for b in range(B)] for c in range(calls)]
        outs, state, _ = _run(rows, n_fft, hop, schedule)
    else:                                                          # every frame in one call, then the flush of both rows
        from avvad import ops
        from avvad.stream import OlaClock
        clock = OlaClock(B, n_fft, hop)
        totals = [R.istft_length(T, n_fft, hop) for T in frames]
        outs, state, per_call = _run(rows, n_fft, hop, [frames], clock=clock, end=False)
        assert per_call == [[T * hop for T in frames]] and clock.ended == [False] * B
        spare = torch.full_like(state, NAN)
        y, n_out = ops.istft_stream(torch.zeros(B, 0, n_fft // 2 + 1, 2, device=DEV), [0] * B, clock, state,
                                    ops.istft_stream_basis(n_fft, DEV), final_samples=totals, out_state=spare)
        assert n_out == [n_fft - hop] * B and y.shape == (B, n_fft - hop)
        outs = [torch.cat([o, y[b]]) for b, o in enumerate(outs)]
        state = spare
    assert torch.count_nonzero(state).item() == 0                 # every row ended: nothing is left
    for b, S in enumerate(rows):
        assert outs[b].shape == (R.istft_length(frames[b], n_fft, hop),)
        if B <= 3 or b in (0, 1, 63, 64, 69):
            _check_row("stream parity %d/%d row %d (%d frames)" % (n_fft, hop, b, frames[b]), outs[b], S.astype(np.complex128), n_fft, hop)


@pytest.mark.parametrize("n_fft,hop,frames", [(64, 16, [9, 4, 1]), (64, 48, [5, 3, 0]), (1024, 256, [37, 5])])
def test_every_split_gives_the_same_bits(n_fft, hop, frames):
    """All frames in one call, one frame per call, and a ragged schedule in which rows advance by different counts, 0
    included: the same samples and the same final state, bit for bit; so does a row alone."""
    rows = _spectra(n_fft, frames, seed=5 + n_fft + hop)
    B, Tm = len(frames), max(frames)
    one = _run(rows, n_fft, hop, [frames])
    each = _run(rows, n_fft, hop, [[1 if c < T else 0 for T in frames] for c in range(Tm)])
    rng = np.random.default_rng(9)
    left, ragged = list(frames), []
    while any(left):
        counts = [int(rng.integers(0, min(l, 4) + 1)) for l in left]
        left = [l - k for l, k in zip(left, counts)]
        ragged.append(counts)
    assert any(0 in c and max(c) > 0 for c in ragged)
    rag = _run(rows, n_fft, hop, ragged)
    for name, got in (("one frame per call", each), ("ragged", rag)):
        for b in range(B):
            assert torch.equal(got[0][b], one[0][b]), "%s, row %d: max|d| = %.3e" % (name, b, float((got[0][b] - one[0][b]).abs().max()))
        assert torch.equal(got[1], one[1]), name
    # and mid-stream, where the state still holds the sums later frames would add to
    per_frame = [[1 if c < T else 0 for T in frames] for c in range(Tm)]
    open_one, open_each = _run(rows, n_fft, hop, [frames], end=False), _run(rows, n_fft, hop, per_frame, end=False)
    assert torch.equal(open_one[1], open_each[1]) and torch.count_nonzero(open_one[1]).item() > 0
    for b in range(B):
        assert torch.equal(open_one[0][b], open_each[0][b]) and torch.equal(open_one[0][b], one[0][b][:frames[b] * hop])
    alone = _run(rows[1:2], n_fft, hop, [[frames[1]]])
    assert torch.equal(alone[0][0], one[0][1])
    if 0 in frames:                                               # a stream that never completes a frame: N zeros at its end
        b = frames.index(0)
        z = _run(rows, n_fft, hop, [frames], totals=[R.istft_length(T, n_fft, hop) if T else 37 for T in frames])[0][b]
        assert z.shape == (37,) and torch.count_nonzero(z).item() == 0 and not torch.signbit(z).any()


def test_mid_stream_state_is_the_partial_sum_and_the_scale_multiplies():
    from avvad import ops
    from avvad.stream import OlaClock
    n_fft, hop = 64, 16
    rows = _spectra(n_fft, [6, 6], seed=2)
    clock = OlaClock(2, n_fft, hop)
    outs, state, _ = _run(rows, n_fft, hop, [[2, 3]], clock=clock, end=False)
    assert torch.count_nonzero(state[:, n_fft - hop:]).item() == 0 and torch.count_nonzero(state[:, :n_fft - hop]).item() > 0
    plain = _run(rows, n_fft, hop, [[2, 3], [4, 3]])[0]
    scale = torch.tensor([2.5, 0.3], device=DEV)
    scaled = _run(rows, n_fft, hop, [[2, 3], [4, 3]], scale=scale)[0]
    for b in range(2):
        assert torch.equal(scaled[b], plain[b] * scale[b])        # one float32 multiplication, nothing else
    _check_row("stream scale 0.3", scaled[1], rows[1].astype(np.complex128), n_fft, hop, scale=float(np.float32(0.3)))
    # counts that do not fit the buffers are refused before the clock moves
    basis = ops.istft_stream_basis(n_fft, DEV)
    st = ops.istft_stream_state(2, n_fft, DEV)
    before = (list(clock.emitted), list(clock.written))
    from avvad import AvvadError
    spec = torch.zeros(2, 2, n_fft // 2 + 1, 2, device=DEV)
    for kw in (dict(frames=[3, 0]), dict(frames=[1]), dict(frames=[1, 1], mask=torch.zeros(2, 2, 5, device=DEV)),
               dict(frames=[1, 1], mask_mode=2), dict(frames=[1, 1], scale=torch.ones(3, device=DEV)),
               dict(frames=[1, 1], out_state=torch.zeros(2, 32, device=DEV)), dict(frames=[1, 1], final_samples={0: 3})):
        with pytest.raises(AvvadError):
            ops.istft_stream(spec, kw.pop("frames"), clock, st, basis, **kw)
        assert (clock.emitted, clock.written) == before
    with pytest.raises(AvvadError):
        ops.istft_stream(spec, [1, 1], clock, st, ops.istft_stream_basis(128, DEV))


@pytest.mark.parametrize("n_fft,hop,frames", [(64, 16, [9, 4]), (1024, 256, [6])])
def test_mask_modes(n_fft, hop, frames):
    """Modes 1, 2 and 3 against the oracle of the float64-masked spectrum, in three calls; mode 3 is bit-equal to mode 1
    with the 0/1 mask of the same logits."""
    rows = _spectra(n_fft, frames, seed=7 + n_fft)
    rng = np.random.default_rng(n_fft)
    B, F = len(frames), n_fft // 2 + 1
    mask = [rng.random((T, F)).astype(np.float32) for T in frames]
    logit = [_logits(rng, (T, F)) for T in frames]
    hard = [(z > 0).astype(np.float32) for z in logit]
    assert 0.2 < np.concatenate(hard).mean() < 0.8
    schedule = [[_split(T, 3)[c] for T in frames] for c in range(3)]
    outs = {1: _run(rows, n_fft, hop, schedule, masks=mask, mode=1)[0], 2: _run(rows, n_fft, hop, schedule, masks=logit, mode=2)[0],
            3: _run(rows, n_fft, hop, schedule, masks=logit, mode=3)[0]}
    soft64 = [1.0 / (1.0 + np.exp(-z.astype(np.float64))) for z in logit]
    for mode, m64 in ((1, [m.astype(np.float64) for m in mask]), (2, soft64), (3, [h.astype(np.float64) for h in hard])):
        for b, S in enumerate(rows):
            _check_row("stream mask mode %d %d/%d row %d" % (mode, n_fft, hop, b), outs[mode][b], S.astype(np.complex128) * m64[b],
                       n_fft, hop)
    as_mask = _run(rows, n_fft, hop, schedule, masks=hard, mode=1)[0]
    default = _run(rows, n_fft, hop, schedule, masks=hard)[0]                     # a mask without a mode: mode 1
    for b in range(B):
        assert torch.equal(outs[3][b], as_mask[b]) and torch.equal(default[b], as_mask[b])
        assert not torch.equal(outs[3][b], outs[2][b])


def test_idle_rows_and_resets():
    """An idle row keeps whatever its state holds, bit for bit, and emits nothing; a row reset mid-batch gives the bits of
    a fresh state beside rows that continue."""
    from avvad import ops
    n_fft, hop = 64, 16
    a, x, y = _spectra(n_fft, [8, 3, 5], seed=31)
    state = ops.istft_stream_state(3, n_fft, DEV)
    state[1] = torch.randn(n_fft, device=DEV)
    kept = state[1].clone()
    # row 0 streams `a` throughout; row 1 idles; row 2 takes 3 frames of x, is reset, and streams y
    schedule = [[2, 0, 2], [1, 0, 1], [2, 0, 2], [3, 0, 3]]
    outs, last, per_call = _run([a, None, x], n_fft, hop, schedule, totals=[R.istft_length(8, n_fft, hop), 0, R.istft_length(5, n_fft, hop)],
                                state=state, resets={2: ([2], [y])})
    assert all(n[1] == 0 for n in per_call) and outs[1].numel() == 0 and torch.equal(last[1], kept)
    assert torch.equal(outs[0], _run([a], n_fft, hop, [[8]])[0][0])
    assert torch.equal(outs[2], _run([y], n_fft, hop, [[5]])[0][0])
    _check_row("stream row reset mid-batch", outs[2], y.astype(np.complex128), n_fft, hop)


# --------------------------------------------------------------------------- samples in, samples out
LENS = [5000, 5120, 3000, 700]     # the end-pad branch of the frame count; no pad; short of the pitch; no frame at all
_PACKETS = {}


def _waves():
    rng = np.random.default_rng(11)
    x = np.zeros((len(LENS), max(LENS)), dtype=np.float32)
    for b, n in enumerate(LENS):
        v = rng.standard_normal(n)
        x[b, :n] = v / np.abs(v).max()
    return x


def _round_trip(packet, n_fft=1024, hop=256):
    """LENS through ops.stft_stream(return_spec=True) + ops.istft_stream (mask mode 0) in packets of ``packet`` samples,
    computed once per packet size -> (samples per row, spectrum per row, features per row)"""
    if packet in _PACKETS:
        return _PACKETS[packet]
    from avvad import ops
    from avvad.stream import OlaClock, SampleClock
    B = len(LENS)
    x = np.full((B, max(LENS) + packet), NAN, dtype=np.float32)      # NaN behind each row's samples: nothing there may be read
    for b, n in enumerate(LENS):
        x[b, :n] = _waves()[b, :n]
    x = T_(x).to(DEV)
    sc, oc = SampleClock(B, n_fft, hop), OlaClock(B, n_fft, hop)
    fb, ib = ops.stft_stream_basis(n_fft, DEV), ops.istft_stream_basis(n_fft, DEV)
    fs, fspare = ops.stft_stream_state(B, n_fft, DEV), torch.full((B, n_fft), NAN, device=DEV)
    os_, ospare = ops.istft_stream_state(B, n_fft, DEV), torch.full((B, n_fft), NAN, device=DEV)
    outs, specs, feats = [[] for _ in range(B)], [[] for _ in range(B)], [[] for _ in range(B)]
    for s0 in range(0, max(LENS), packet):
        n = [min(max(l - s0, 0), packet) for l in LENS]
        fin = [b for b in range(B) if 0 < LENS[b] - s0 <= packet]
        chunk = x[:, s0:s0 + packet].contiguous()
        f, frames, spec = ops.stft_stream(chunk, n, sc, fs, fb, final=fin, out_state=fspare, return_spec=True)
        fs, fspare = fspare, fs
        assert spec.shape == (B, max(frames), n_fft // 2 + 1, 2)
        for b in range(B):
            assert torch.count_nonzero(spec[b, frames[b]:]).item() == 0
        if max(frames) == 0 and not fin:
            continue
        y, n_out = ops.istft_stream(spec, frames, oc, os_, ib, final_samples={b: LENS[b] for b in fin}, out_state=ospare)
        os_, ospare = ospare, os_
        for b in range(B):
            outs[b].append(y[b, :n_out[b]])
            specs[b].append(spec[b, :frames[b]])
            feats[b].append(f[b, :frames[b]])
    assert oc.written == LENS and torch.count_nonzero(os_).item() == 0
    _PACKETS[packet] = ([torch.cat(o) for o in outs], [torch.cat(s) for s in specs], [torch.cat(f) for f in feats])
    return _PACKETS[packet]


@pytest.mark.parametrize("packet", [1, 160, 2500])
def test_final_flush_returns_exactly_the_samples_that_went_in(packet):
    """Every row returns exactly N samples, the three packetings give the same bits, mask mode 0 returns the input on the
    samples every frame position covers (the rule and helper of test_round_trip_returns_the_waveform), and the stream that
    completes no frame is all zeros."""
    from avvad import ops
    n_fft, hop = 1024, 256
    x = _waves()
    outs, specs, _ = _round_trip(packet)
    ref_outs, ref_specs, _ = _round_trip(160)
    for b, n in enumerate(LENS):
        assert outs[b].shape == (n,)
        assert torch.equal(outs[b], ref_outs[b]) and torch.equal(specs[b], ref_specs[b]), (packet, b)
        T = max(ops.n_frames(n, n_fft, hop), 0)
        assert specs[b].shape[0] == T
        if T == 0:
            assert torch.count_nonzero(outs[b]).item() == 0 and not torch.signbit(outs[b]).any()
            continue
        natural = R.istft_length(T, n_fft, hop)
        y32 = R.istft32_gemm(R.stft32_gemm(x[b, :n], n_fft, hop), n_fft, hop)
        g32, ref = _covered(y32, x[b], n, natural, hop)
        e32 = float(np.abs(g32 - ref).max())
        got, ref = _covered(outs[b].cpu().numpy(), x[b], n, natural, hop)
        print("istft stream: round trip L = %d packets of %d  E = %.3e  E_cpu32 = %.3e" % (n, packet, np.abs(got - ref).max(), e32))
        _ireport("stream round trip L = %d, packets of %d" % (n, packet), got, ref, R.FACTOR * e32)


def _feature_bound():
    """(atol, rtol) test_stft_stream_gpu.py holds the streamed features to against ops.stft, read from that file"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_stft_stream_gpu.py")).read()
    m = re.search(r'_report\("features around a silence vs ops\.stft", got, whole, ([0-9.e+-]+), ([0-9.e+-]+)\)', src)
    assert m, "the feature bound of test_stft_stream_gpu.py moved"
    return float(m.group(1)), float(m.group(2))


def test_return_spec():
    """The spectrum is bit-identical across packetings (test_final_flush...), its features are bit-equal to the call without
    return_spec, and it is within ops.stft_complex of the whole utterance under test_stft_stream_gpu.py's feature bound."""
    from avvad import ops
    from avvad.stream import SampleClock
    from test_stft_stream_gpu import _const, _stream_rows
    from test_stft_stream_gpu import _report as _sreport
    n_fft, hop = 1024, 256
    x = T_(_waves()).to(DEV)
    _, specs, feats = _round_trip(160)
    plain = _stream_rows([x[b, :n] for b, n in enumerate(LENS)], [_const(160)] * len(LENS))[0]
    atol, rtol = _feature_bound()
    for b, n in enumerate(LENS):
        assert torch.equal(feats[b], plain[b]), b
        if specs[b].shape[0]:
            whole = ops.stft_complex(x[b, :n].contiguous(), n_fft, hop)[0]
            _sreport("spectrum vs ops.stft_complex, L = %d" % n, specs[b], whole, atol, rtol)
    # the peak divides the samples the spectrum is of
    c = SampleClock(1, n_fft, hop)
    st = ops.stft_stream_state(1, n_fft, DEV)
    basis = ops.stft_stream_basis(n_fft, DEV)
    a = ops.stft_stream(x[:1, :2048].contiguous(), None, c, st, basis, peak=torch.tensor([2.0], device=DEV), return_spec=True)[2]
    c.reset()
    st.zero_()
    h = ops.stft_stream((x[:1, :2048] / 2.0).contiguous(), None, c, st, basis, return_spec=True)[2]
    assert a.shape == (1, 5, 513, 2) and torch.equal(a, h)


# --------------------------------------------------------------------------- the session
def _model(ydim=513):
    from packages.models.Audio_Net import DeepVAD_audio
    m = DeepVAD_audio(2, 32, ydim)
    m.load_state_dict(torch.load(os.path.join(GOLDEN, "audio_ref_h32_y%d.pt" % ydim), map_location="cpu", weights_only=True))
    return m.to(DEV).eval()


def _utt(n=6000, start=12000):
    from avvad import train as TR
    x, fs = TR.load_waveform(os.path.join(GOLDEN, "utt_sa1.npz"))
    assert fs == 16000
    return x[start:start + n].contiguous()


def _enhance(sess, x, packet, hard):
    """x (1, N) through step_enhance in packets -> (logits (T, F), samples (N,))"""
    N = x.shape[1]
    logits, outs = [], []
    for s0 in range(0, N, packet):
        lg, fr, y, k = sess.step_enhance(x[:, s0:s0 + packet].contiguous(), final=[0] if s0 + packet >= N else None, hard=hard)
        assert lg.shape[1] == fr[0] and y.shape == (1, k[0])
        logits.append(lg[0, :fr[0]])
        outs.append(y[0, :k[0]])
    return torch.cat(logits), torch.cat(outs)


def test_session_step_enhance_against_the_oracle_and_ops_resynth():
    """A 6000-sample utterance in packets of 400 with the soft mask of the reference's 513-output checkpoint: the samples
    that come out, and ops.resynth of the whole peak-normalised wave with the session's own logits as the mode-2 mask, are
    float32 evaluations of istft64(stft64(x) * sigmoid(logits)); both are held to 8 E_cpu32 of it."""
    from avvad import ops, stream, train as TR
    g = load_golden("eval_audio")
    stats = TR.Stats(audio_mean=g["mean"], audio_std=g["std"])
    n_fft, hop, N = 1024, 256, 6000
    x = _utt(N).to(DEV).view(1, -1)
    sess = stream.open(_model(), 1)
    sess.set_frontend(stats)
    peak = ops.peak(x)
    sess.peak.copy_(peak)
    logits, y = _enhance(sess, x, 400, hard=False)
    T = ops.n_frames(N, n_fft, hop)
    assert logits.shape == (T, 513) and y.shape == (N,) and bool(torch.isfinite(y).all())
    assert sess.ola_clock.written == [N] and torch.count_nonzero(sess.ola_state).item() == 0
    xn = x / peak                                                 # the division the session's front-end does per sample
    whole = ops.resynth(xn, logits.view(1, T, 513).contiguous(), mask_mode=2, n_fft=n_fft, hop=hop, scale=peak)[0]
    assert whole.shape == (N,)
    xn_np, z = xn[0].cpu().numpy(), logits.cpu().numpy()
    soft64 = 1.0 / (1.0 + np.exp(-z.astype(np.float64)))
    _, num, wss = R.istft64(R.stft64(xn_np, n_fft, hop) * soft64, n_fft, hop, length=N)
    soft32 = (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    y32 = R.istft32_gemm(R.stft32_gemm(xn_np, n_fft, hop) * np.repeat(soft32, 2, axis=1), n_fft, hop, length=N)
    e32 = R.weighted_error(y32, num, wss)[0]
    assert e32 > 0
    pk = float(peak.item())
    for name, got in (("session step_enhance", y), ("ops.resynth, the session's logits", whole)):
        e, gw, ref = R.weighted_error(got.cpu().numpy(), num, wss, pk)
        print("istft stream: %-36s E = %.3e  E_cpu32 = %.3e  ratio %.2f" % (name, e / pk, e32, e / pk / e32))
        _ireport(name + " vs float64", gw, ref, R.FACTOR * e32 * pk)


def test_session_hard_mask_mixing_and_models_without_a_mask():
    from avvad import AvvadError, stream
    x = _utt(6000).to(DEV).view(1, -1)
    m = _model()
    runs = []
    for _ in range(2):
        sess = stream.open(m, 1)
        runs.append(_enhance(sess, x, 400, hard=True))
        assert runs[-1][1].shape == (6000,) and bool(torch.isfinite(runs[-1][1]).all())
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # a live row stays with the route it took
    sess = stream.open(m, 2)
    w = torch.randn(2, 1500, device=DEV) * 0.1
    sess.step_enhance(w, samples=[1500, 0])
    keep = lambda: (sess.h.clone(), sess.c.clone(), sess.stft_state.clone(), sess.ola_state.clone(),      # noqa: E731
                    list(sess.sample_clock.total), list(sess.ola_clock.written), list(sess._route))
    before = keep()
    with pytest.raises(AvvadError, match="step_enhance"):
        sess.step_wave(w)
    after = keep()
    assert all(torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b for a, b in zip(before, after))
    sess.step_wave(w, samples=[0, 700])                          # the row that has taken nothing may go either way
    with pytest.raises(AvvadError, match="step_wave"):
        sess.step_enhance(w, samples=[100, 100])
    sess.reset([1])
    lg, fr, y, k = sess.step_enhance(w, samples=[100, 1500])
    assert fr == [1, 2] and k == [256, 512] and y.shape == (2, 512)
    sess.set_frontend(n_fft=512, hop=128)                         # a new framing drops the states
    assert sess.ola_state is None and sess.stft_state is None and sess.ola_clock.n_fft == 512
    with pytest.raises(AvvadError, match="mask"):
        sess.step_enhance(w)                                      # 513 outputs mask no 257 bins
    with pytest.raises(AvvadError, match="mask"):
        stream.open(_model(1), 1).step_enhance(w[:1])


def test_evaluator_writes_the_streamed_enhanced_utterance(tmp_path):
    from scipy.io import wavfile
    from avvad import train as TR
    from packages.models.Audio_Net import DeepVAD_audio
    g = load_golden("eval_audio")
    wav = os.path.join(GOLDEN, "utt_sa1.npz")
    ck = os.path.join(GOLDEN, "audio_ref_h32_y513.pt")
    stats = TR.Stats(audio_mean=g["mean"], audio_std=g["std"])
    make = lambda: DeepVAD_audio(2, 32, 513)      # noqa: E731
    TR.evaluate_main("audio", make, checkpoint=ck, out_dir=str(tmp_path / "a"), wav_list=[wav], stats=stats,
                     resynth_dir=str(tmp_path / "wav"), chunk_samples=400, resynth_chunked=True, resynth_hard=False)
    assert os.listdir(tmp_path / "wav") == ["utt_sa1_enhanced.wav"]
    fs, y = wavfile.read(str(tmp_path / "wav" / "utt_sa1_enhanced.wav"))
    x_t, _ = TR.load_waveform(wav)
    assert fs == 16000 and y.dtype == np.float32 and y.shape == (x_t.numel(),) == (48100,)
    assert np.isfinite(y).all() and np.abs(y).max() > 0
    model = make()
    model.load_state_dict(torch.load(ck, map_location="cpu", weights_only=True))
    model = model.to(DEV).eval()
    with torch.no_grad():
        direct = TR.resynth_utt(model, x_t.to(DEV), stats, hard=False, chunk_samples=400)
        whole = TR.resynth_utt(model, x_t.to(DEV), stats, hard=False)
    assert np.array_equal(direct.cpu().numpy(), y)
    assert whole.shape == direct.shape
    print("istft stream: enhanced utt_sa1 peak %.3f, max|streamed - whole utterance| = %.3e away from the ends"
          % (np.abs(y).max(), float((direct - whole)[1024:-1024].abs().max())))


@pytest.mark.parametrize("n_fft", [32, 64])
def test_streaming_inverse_basis_is_the_whole_utterance_basis(n_fft):
    """Frame c of the spectrum is a unit impulse at packed contraction row c of the streaming kernel (c = 0: re[0], c = 1:
    re[n_fft/2], c = 2f, 2f + 1: re[f], im[f] for 1 <= f < n_fft/2; never im[0] or im[n_fft/2]) and hop = n_fft, so no two
    frames overlap: every sum of the whole-utterance inverse and of the streaming one is one product 1.0 * W plus exact
    zeros, divided by the same (float) hann^2[n] (or not at all where that is not above FLT_MIN, n = 0).  The two hold the
    same basis floats exactly when the two outputs are the same bits."""
    from avvad import ops
    from avvad.stream import OlaClock
    N, F = n_fft, n_fft // 2 + 1
    spec = torch.zeros(1, N, F, 2, device=DEV)
    spec[0, 0, 0, 0] = 1.0
    spec[0, 1, N // 2, 0] = 1.0
    for f in range(1, N // 2):
        spec[0, 2 * f, f, 0] = 1.0
        spec[0, 2 * f + 1, f, 1] = 1.0
    assert int(spec.count_nonzero()) == N and not spec[0, :, 0, 1].any() and not spec[0, :, N // 2, 1].any()
    whole = ops.istft(spec, N, N, center=False)
    stream, n_out = ops.istft_stream(spec, [N], OlaClock(1, N, N), ops.istft_stream_state(1, N, DEV), ops.istft_stream_basis(N, DEV))
    assert n_out == [N * N] and whole.shape == stream.shape == (1, N * N)
    assert whole.any()
    assert torch.equal(whole, stream)
