"""The resampler on the GPU (csrc/resample.hip): values against the float64 restatement of tests/resample_ref.py under its
derived bound, then the exact properties -- a row alone, run to run, under "max_cus", every split of a stream, a stream
against the whole utterance: the same bits -- and the layers above it: the session at 48 and 44.1 kHz and the training
and evaluation paths with ``resample=True``.  Each value test prints its largest error in units of the bound (0.87 .. 0.98 on
the rows of a tile or more: the float32 rounding term is what is nearly reached)."""
import functools
import random

import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
# the issue's six, then two whose input span is beyond what a workgroup stages in LDS (decimation by more than about 29):
# 1/40 with its taps in LDS, 7/300 with 6 006 taps read from global memory -- the kernel's other two forms
RATIOS = [(1, 3), (2, 1), (5, 8), (160, 441), (800, 999), (1, 6), (1, 40), (7, 300)]


def _tile():
    from avvad import _lib as L
    return L.RESAMPLE_TILE


def _inputs_for(n_out, up, down, exactly):
    """the largest input length that gives ``exactly`` n_out outputs, or the smallest that gives at least n_out (with
    up > down not every count occurs)"""
    Ls = range(1, n_out * down // up + down + 2)
    return max(L for L in Ls if R.length(L, up, down) == n_out) if exactly else min(L for L in Ls if R.length(L, up, down) >= n_out)


@functools.lru_cache(maxsize=None)
def _ragged(up, down):
    """The ragged batch of the value test, its float64 reference and the GPU result: built once per ratio.
    -> (lens, rows (numpy float32), refs [(ref, A)], out (B, Lout) on the CPU, n_out)"""
    from avvad import ops
    T = _tile()
    lens = [1, 7, _inputs_for(T, up, down, True), _inputs_for(T + 1, up, down, False), _inputs_for(2 * T + 77, up, down, False)]
    rng = np.random.default_rng(up * 1000 + down)
    rows = [rng.standard_normal(n).astype(np.float32) for n in lens]
    Lmax, pitch = max(lens), max(lens) + 13
    big = torch.full((len(lens) * pitch + 8,), NAN, dtype=torch.float32, device=DEV)
    x = big[1:1 + len(lens) * pitch].view(len(lens), pitch)       # a row pitch behind L, the base 4 bytes off 16
    assert x.data_ptr() % 16 == 4
    for b, r in enumerate(rows):
        x[b, :len(r)] = torch.from_numpy(r).to(DEV)                # NaN behind every length
    out, n_out = ops.resample(x[:, :Lmax], lens, fs_in=down, fs_out=up)
    refs = [R.resample(r, up, down) for r in rows]
    return lens, rows, refs, out.cpu(), n_out


def _assert_within(got, ref, A, up, down, what):
    err = np.abs(got.astype(np.float64) - ref)
    tol = R.tol(ref, A, up, down)
    worst = float((err / np.maximum(tol, 1e-300)).max()) if len(ref) else 0.0
    print("resample %d/%d %s: max err / tol = %.3f over %d outputs" % (up, down, what, worst, len(ref)))
    assert np.all(err <= tol), (what, worst)


@pytest.mark.parametrize("up,down", RATIOS)
def test_whole_utterance_values_counts_and_tail(up, down):
    lens, rows, refs, out, n_out = _ragged(up, down)
    Lout = R.length(max(lens), up, down)
    assert out.shape == (len(lens), Lout)
    assert n_out == [R.length(n, up, down) for n in lens]
    assert n_out[2] == _tile() < n_out[3] <= _tile() + up and 2 * _tile() + 77 <= n_out[4] < 2 * _tile() + 77 + up
    for b, (ref, A) in enumerate(refs):
        got = out[b].numpy()
        assert np.all(np.isfinite(got))
        _assert_within(got[:n_out[b]], ref, A, up, down, "row %d (L = %d)" % (b, lens[b]))
        assert np.all(got[n_out[b]:].view(np.int32) == 0)         # +0 from the row's count to Lout


@pytest.mark.parametrize("up,down", RATIOS)
def test_a_row_alone_run_to_run_and_under_max_cus(up, down, lib_options):
    from avvad import ops
    lens, rows, refs, out, n_out = _ragged(up, down)
    for b, r in enumerate(rows):
        alone, n1 = ops.resample(torch.from_numpy(r).to(DEV), fs_in=down, fs_out=up)
        assert alone.dim() == 1 and n1 == [n_out[b]]
        assert torch.equal(alone.cpu(), out[b, :n_out[b]]), b
    x = torch.zeros(len(lens), max(lens), device=DEV)
    for b, r in enumerate(rows):
        x[b, :len(r)] = torch.from_numpy(r).to(DEV)
    again = ops.resample(x, lens, fs_in=down, fs_out=up)[0]
    assert torch.equal(again.cpu(), out)
    lib_options("max_cus", 8)
    assert torch.equal(ops.resample(x, lens, fs_in=down, fs_out=up)[0].cpu(), out)


def test_same_rate_returns_the_input_and_bad_arguments_raise():
    from avvad import ops
    from avvad._lib import AvvadError
    x = torch.randn(2, 50, device=DEV)
    y, n = ops.resample(x, [50, 20], fs_in=16000)
    assert y is x and n == [50, 20]
    with pytest.raises(AvvadError, match="fs_in"):
        ops.resample(x)
    with pytest.raises(AvvadError, match="lengths"):
        ops.resample(x, [51, 3], fs_in=48000)
    with pytest.raises(AvvadError, match="GPU"):
        ops.resample(x.cpu(), fs_in=48000)
    with pytest.raises(AvvadError, match="16001"):
        ops.resample(x, fs_in=16001)


# ------------------------------------------------------------------------------------------------ the streamed form
def _feed(rows, packets, up, down, clock=None, state=None, resets=()):
    """Feeds row b its ``packets[b]`` (sizes, one per call; a row whose list is spent idles), the last one final.  Chunks
    are padded with NaN behind a row's samples.  ``resets``: {(call, row): new 1-D tensor and its packets} starts another
    utterance on that row before that call, the state left as it is.  -> (per-row outputs (1-D, CPU), clock, state)"""
    from avvad import ops
    from avvad.stream import RateClock
    B = len(rows)
    rows, packets = list(rows), [list(p) for p in packets]
    clock = RateClock(B, up, down) if clock is None else clock
    taps = ops.resample_taps_on(up, down, DEV)
    state = ops.resample_stream_state(B, up, down, DEV) if state is None else state
    spare = torch.full_like(state, NAN)
    at, pos, outs, call = [0] * B, [0] * B, [[] for _ in range(B)], 0
    resets = dict(resets)
    while any(at[b] < len(packets[b]) for b in range(B)) or any(c >= call for c, _ in resets):
        for (c, b), (row, pk) in list(resets.items()):
            if c == call:
                clock.reset([b])
                state[b].fill_(NAN)                           # in front of a reset nothing is read
                rows[b], packets[b], at[b], pos[b], outs[b] = row, list(pk), 0, 0, []
                del resets[(c, b)]
        n = [packets[b][at[b]] if at[b] < len(packets[b]) else 0 for b in range(B)]
        fin = [b for b in range(B) if at[b] == len(packets[b]) - 1]
        chunk = torch.full((B, max(n)), NAN, dtype=torch.float32, device=DEV)
        for b in range(B):
            if n[b]:
                chunk[b, :n[b]] = rows[b][pos[b]:pos[b] + n[b]]
        before = state.clone()
        plan = clock.plan(n, fin)
        out, k = ops.resample_stream(chunk, n, clock, state, taps, fin, spare)
        assert k == plan and out.shape == (B, max(k))
        state, spare = spare, state
        for b in range(B):
            if n[b] == 0 and b not in fin:                    # a row with nothing to do copies its state
                assert torch.equal(state[b].view(torch.int32), before[b].view(torch.int32))
            assert np.all(out[b, k[b]:].cpu().numpy().view(np.int32) == 0)
            outs[b].append(out[b, :k[b]].cpu())
            pos[b] += n[b]
            at[b] += 1 if at[b] < len(packets[b]) else 0
        call += 1
    return [torch.cat(o) if o else torch.zeros(0) for o in outs], clock, state


def _mixed_packets(seed):
    rnd = random.Random(seed)
    p = [rnd.choice([0, 1, 7, 441, 1000]) for _ in range(14)] + [0, 1, 7, 441, 1000]
    rnd.shuffle(p)
    return p


@pytest.mark.parametrize("up,down", [(1, 3), (160, 441), (2, 1)])
@pytest.mark.parametrize("schedule", ["ones", "mixed", "one packet"])
def test_streamed_equals_whole_bit_for_bit(up, down, schedule):
    from avvad import ops
    packets = {"ones": [1] * 700, "mixed": _mixed_packets(up + down), "one packet": [2500]}[schedule]
    x = torch.randn(sum(packets), device=DEV)
    whole, n = ops.resample(x, fs_in=down, fs_out=up)
    (got,), clock, _ = _feed([x], [packets], up, down)
    assert got.numel() == n[0] == clock.emitted[0]
    assert torch.equal(got, whole.cpu())


def test_rows_that_end_at_different_calls_a_reset_and_an_idle_row():
    from avvad import ops
    up, down = 160, 441
    a, b, c, b2 = (torch.randn(n, device=DEV) for n in (1500, 900, 1200, 777))
    packets = [[500, 500, 500], [450, 450], [600, 0, 0, 0, 600]]
    got, clock, _ = _feed([a, b, c], packets, up, down, resets={(3, 1): (b2, [77, 700])})
    for g, x in zip(got, (a, b2, c)):
        whole = ops.resample(x, fs_in=down, fs_out=up)[0].cpu()
        assert torch.equal(g, whole)
    # the first utterance of row 1, cut off by the reset, on its own
    (gb,), _, _ = _feed([b], [[450, 450]], up, down)
    assert torch.equal(gb, ops.resample(b, fs_in=down, fs_out=up)[0].cpu())
    from avvad._lib import AvvadError
    with pytest.raises(AvvadError, match="reset"):
        clock.plan([1, 0, 0])


def test_a_clock_preset_to_three_billion_samples():
    """64-bit positions: the row stands 3 000 000 000 inputs into its stream (everything before is silence)."""
    from avvad import ops
    from avvad.stream import RateClock
    start = 3_000_000_000
    for up, down in ((1, 3), (160, 441)):
        x = np.random.default_rng(7).standard_normal(900).astype(np.float32)
        packets = [400, 1, 499]
        ref, A, _ = R.stream(x, packets, up, down, start=start)
        clock = RateClock(1, up, down)
        clock.preset(0, start)
        assert clock.emitted[0] == R.emitted(start, up, down) and clock.emitted[0] * down > 2 ** 31
        (got,), clock, _ = _feed([torch.from_numpy(x).to(DEV)], [packets], up, down, clock=clock)
        assert clock.total[0] == start + 900 and clock.emitted[0] == R.length(start + 900, up, down)
        _assert_within(got.numpy(), ref, A, up, down, "at 3e9")
        assert float(np.abs(ref).max()) > 0.1


# ------------------------------------------------------------------------------------------------ the session
def _tiny_audio(ydim):
    from packages.models.Audio_Net import DeepVAD_audio
    torch.manual_seed(3)
    return DeepVAD_audio(1, 16, ydim).to(DEV).eval()


@pytest.mark.parametrize("fs_in", [48000, 44100])
def test_session_logits_equal_resampling_the_whole_utterance(fs_in):
    from avvad import ops, stream
    m = _tiny_audio(1)
    x = 0.3 * torch.randn(1, fs_in // 4, device=DEV)
    N = x.shape[1]
    x16, (n16,) = ops.resample(x, fs_in=fs_in)
    ref_s = stream.open(m, 1)
    ref, fr_ref = ref_s.step_wave(x16, final=[0])
    assert fr_ref == [ops.n_frames(n16, 1024, 256)]
    for size in (480, 1111):
        s = stream.open(m, 1)
        s.set_frontend(fs_in=fs_in)
        parts = []
        for s0 in range(0, N, size):
            n = min(size, N - s0)
            fin = [0] if s0 + size >= N else []
            plan = s.plan_wave([n], fin)
            y, fr = s.step_wave(x[:, s0:s0 + n].contiguous(), final=fin)
            assert fr == plan
            parts.append(y[:, :fr[0]])
        got = torch.cat(parts, dim=1)
        assert got.shape == ref.shape and torch.equal(got, ref)
        s.reset()                                                # a second utterance on the same session
        y, fr = s.step_wave(x, final=[0])
        assert torch.equal(y, ref)
        s.set_frontend(fs_in=16000)                              # back at 16 kHz the resampler is out of the path
        s.reset()                                                # (the front-end started over; the LSTM state is reset's)
        assert s.rate_clock is None
        y, fr = s.step_wave(x16, final=[0])
        assert torch.equal(y, ref)


@pytest.mark.parametrize("fs_in", [48000, 44100])
def test_step_enhance_returns_resample_length_samples(fs_in):
    from avvad import ops, stream
    m = _tiny_audio(513)
    N = 9000
    x = 0.3 * torch.randn(2, N, device=DEV)
    lens = [N, 5000]
    up, down = ops.resample_ratio(fs_in)
    s = stream.open(m, 2)
    s.set_frontend(fs_in=fs_in)
    total, ended = [0, 0], set()
    for s0 in range(0, N, 2000):
        n = [min(max(l - s0, 0), 2000) for l in lens]
        fin = [b for b in range(2) if b not in ended and s0 + 2000 >= lens[b]]
        ended.update(fin)
        _, _, enh, k = s.step_enhance(x[:, s0:s0 + 2000].contiguous(), n, None, fin)
        assert enh.shape == (2, max(k))
        total = [t + kk for t, kk in zip(total, k)]
    assert total == [ops.resample_length(l, up, down) for l in lens]


# ------------------------------------------------------------------------------------------------ training and evaluation paths
def _npz(path, n, fs, seed):
    x = (np.random.default_rng(seed).standard_normal(n) * 3000).astype(np.int16)
    np.savez(path, samples=x, fs=fs)
    return str(path)


def _files(tmp_path):
    """tiny utterances of 48, 16 and 8 kHz, about 0.2 s each, and two noise clips"""
    utt = [_npz(tmp_path / "u48.npz", 9000, 48000, 1), _npz(tmp_path / "u16.npz", 3300, 16000, 2),
           _npz(tmp_path / "u8.npz", 1700, 8000, 3)]
    noise = [_npz(tmp_path / "n48.npz", 7000, 48000, 4), _npz(tmp_path / "n16.npz", 2500, 16000, 5)]
    return utt, noise


def _as_16k(path):
    from avvad import ops, train as TR
    x, fs = TR.load_waveform(path)
    return ops.resample(x.to(DEV), fs_in=fs)[0].cpu()


def test_noise_bank_and_steps_equal_the_same_calls_on_resampled_tensors(tmp_path):
    from avvad import ops, train as TR
    utt, noise = _files(tmp_path)
    bank = TR.read_noise_bank(noise, DEV, resample=True)
    want = ops.NoiseBank([_as_16k(p) for p in noise], DEV)
    assert bank.lengths == want.lengths == [ops.resample_length(7000, 1, 3), 2500]
    assert all(torch.equal(getattr(bank, k), getattr(want, k)) for k in ("data", "clip_off", "clip_len"))
    u16 = [_as_16k(p) for p in utt]
    draw = lambda n: ([0, 1, 0], [5, 7, 11], [3.0, -2.0, 10.0])        # noqa: E731
    # mix_step: a batch that carries rates against the same utterances resampled beforehand
    ds = TR.CleanWavs(utt, resample=True)
    got = TR.mix_step(TR.CleanWavs.collate([ds[i] for i in range(3)]), DEV, "ibm_labels", bank, draw, waves=True)
    ref = TR.mix_step(TR.CleanWavs.collate([(u, u.numel()) for u in u16]), DEV, "ibm_labels", want, draw, waves=True)
    assert got[3][2] == ref[3][2] == [u.numel() for u in u16]
    for a, b in zip(got[:3] + got[3][:2] + got[3][3:], ref[:3] + ref[3][:2] + ref[3][3:]):
        assert torch.equal(a, b)
    # wav_pair_step: pairs whose two files differ in rate and in length, cropped to their common length after resampling
    pairs = [(utt[0], utt[1]), (utt[2], utt[0]), (utt[1], utt[1])]
    dp = TR.WavPairs(pairs, resample=True)
    got = TR.wav_pair_step(TR.WavPairs.collate([dp[i] for i in range(3)]), DEV, "vad_labels", waves=True)
    items = []
    for a, b in ((0, 1), (2, 0), (1, 1)):
        n = min(u16[a].numel(), u16[b].numel())
        items.append((u16[a][:n], u16[b][:n], n))
    ref = TR.wav_pair_step(TR.WavPairs.collate(items), DEV, "vad_labels", waves=True)
    assert got[3][2] == ref[3][2] == [it[2] for it in items]
    for a, b in zip(got[:3] + got[3][:2], ref[:3] + ref[3][:2]):
        assert torch.equal(a, b)


def test_train_main_on_files_of_three_rates(tmp_path):
    import os
    import re
    from avvad import train as TR
    from packages.models.Audio_Net import DeepVAD_audio
    utt, noise = _files(tmp_path)
    out = str(tmp_path / "run")
    TR.train_main("audio", lambda: DeepVAD_audio(1, 16, 513), "rs", epochs=1, batch_size=2, lr=1e-3, out_dir=out,
                  clean_wavs=utt, noise_wavs=noise, snr_db=(0.0, 10.0), mix_seed=1, compute_stats=True, resample=True)
    log = open(os.path.join(out, "output_batch.log")).read()
    losses = [float(v) for v in re.findall(r"loss (\S+)", log)]
    # three utterances in batches of two: two steps; the log holds the first batch's loss and the epoch's train / valid means
    assert len(re.findall(r"Epoch: +1 ", log)) == 1 and len(losses) == 3 and all(np.isfinite(losses)), log
    with pytest.raises(ValueError, match="expected 16 kHz audio"):
        TR.train_main("audio", lambda: DeepVAD_audio(1, 16, 513), "rs", epochs=1, batch_size=2, out_dir=out, clean_wavs=utt,
                      noise_wavs=noise[1:])


def test_evaluate_main_round_trip_on_a_48_khz_file(tmp_path):
    import os
    from scipy.io import wavfile
    from avvad import ops, train as TR
    from packages.models.Audio_Net import DeepVAD_audio
    utt, _ = _files(tmp_path)
    wav = utt[0]
    n16 = ops.resample_length(9000, 1, 3)
    T = ops.n_frames(n16, 1024, 256)
    make = lambda: DeepVAD_audio(1, 16, 513)                         # noqa: E731
    with pytest.raises(ValueError, match="expected 16 kHz audio, got 48000"):
        TR.evaluate_main("audio", make, out_dir=str(tmp_path / "no"), wav_list=[wav])
    outs = {}
    for tag, kw in (("whole", {}), ("chunked", dict(chunk_samples=700, resynth_chunked=True))):
        d = tmp_path / tag
        TR.evaluate_main("audio", make, out_dir=str(d), wav_list=[wav], clean_of={wav: wav}, resynth_dir=str(d / "wav"),
                         score_dir=str(d / "score"), resample=True, **kw)
        soft = torch.load(d / "u48_y_hat_soft.pt", weights_only=True)
        label = torch.load(d / "u48_label.pt", weights_only=True)
        fs, enh = wavfile.read(str(d / "wav" / "u48_enhanced.wav"))
        scores = torch.load(d / "score" / "u48_scores.pt", weights_only=True)
        assert soft.shape == (1, T) and label.shape == (1, T) and fs == 16000 and enh.shape == (n16,)
        assert np.isfinite(scores["si_sdr"]) and bool(torch.isfinite(soft).all())
        outs[tag] = soft
    assert float((outs["whole"] - outs["chunked"]).abs().max()) < 1e-4       # the same values up to summation order
    # the whole route is the 16 kHz evaluator on the resampled utterance, bit for bit
    x16 = _as_16k(wav).to(DEV)
    torch.manual_seed(0)
    model = make().to(DEV).eval()
    soft, _ = TR.process_utt(model, x16, None, T)
    assert torch.equal(soft, outs["whole"])
    soft48, _ = TR.process_utt(model, TR.load_waveform(wav)[0].to(DEV), None, T, fs_in=48000)
    assert torch.equal(soft48, soft)
