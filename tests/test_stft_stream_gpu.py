"""The streaming STFT front-end on the GPU.  Exact properties first -- any split of a stream into calls, any row of any
batch, in place or through a spare state, saved and restored: the same bits -- then the values against the oracle's
whole-utterance front-end and the outputs the reference's own checkpoints produced, under the bounds the
whole-utterance path is held to (features atol 2e-3 + rtol 1e-4, outputs 1e-4).  Observed maxima go to the parity log."""
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

from test_gpu_parity import _report as _parity_report

pytestmark = pytest.mark.gpu
T_ = torch.from_numpy
DEV = "cuda:0"


def _report(name, got, ref, atol, rtol=0.0):
    _parity_report("stft_stream: " + name, got, ref, atol, rtol)


def _utt():
    from avvad import train as TR
    x, fs = TR.load_waveform(os.path.join(GOLDEN, "utt_sa1.npz"))
    assert fs == 16000 and x.numel() == 48100
    return x


def _stats():
    g = load_golden("eval_audio")
    return T_(g["mean"]).reshape(-1).to(DEV), T_(g["std"]).reshape(-1).to(DEV)


def _const(n):
    return lambda call: n


def _stream_rows(rows, sizes, n_fft=1024, hop=256, mean=None, std=None, peak=None, in_place=False, state=None,
                 name_state=False):
    """Feeds ``rows`` (1-D GPU tensors; None: an idle row that gets 0 samples in every call) through ops.stft_stream,
    row b taking ``sizes[b](call)`` samples per call until it runs out; its last packet is final.  The chunk is padded
    with NaN behind each row's valid samples: nothing behind them may be read.
    -> (per-row features (frames, F), the last state, the clock)"""
    from avvad import ops
    from avvad.stream import SampleClock
    B = len(rows)
    basis = ops.stft_stream_basis(n_fft, DEV)
    clock = SampleClock(B, n_fft, hop)
    state = ops.stft_stream_state(B, n_fft, DEV) if state is None else state
    spare = torch.full_like(state, float("nan"))
    left = [0 if r is None else r.numel() for r in rows]
    pos = [0] * B
    outs = [[] for _ in range(B)]
    call = 0
    while any(left):
        n = [min(left[b], int(sizes[b](call))) if rows[b] is not None else 0 for b in range(B)]
        fin = [b for b in range(B) if left[b] > 0 and n[b] == left[b]]
        chunk = torch.full((B, max(max(n), 1)), float("nan"), device=DEV)
        for b in range(B):
            if n[b]:
                chunk[b, :n[b]] = rows[b][pos[b]:pos[b] + n[b]]
        kept = chunk.clone()
        feats, frames = ops.stft_stream(chunk, n, clock, state, basis, peak, mean, std, fin,
                                        (state if name_state else None) if in_place else spare)
        assert torch.equal(torch.nan_to_num(chunk, nan=7.0), torch.nan_to_num(kept, nan=7.0)), "the input chunk was written"
        assert feats.shape == (B, max(frames), n_fft // 2 + 1)
        if not in_place:
            state, spare = spare, state
        for b in range(B):
            outs[b].append(feats[b, :frames[b]])
            assert float(feats[b, frames[b]:].abs().sum()) == 0.0            # the rest of out is zeroed
            pos[b] += n[b]
            left[b] -= n[b]
        call += 1
        assert call < 200000
    return [torch.cat(o, 0) for o in outs], state, clock


def test_split_invariance_bit_for_bit():
    """utt_sa1 with the golden statistics as one call, 160-sample packets, 256-sample packets, 1-sample packets for the
    first 3000 samples then the rest, and seeded random packets in 1..2000: five equal tensors."""
    from avvad import ops
    x = _utt().to(DEV)
    mean, std = _stats()
    rng = random.Random(5)
    splits = {"one call": _const(1 << 30), "160": _const(160), "256": _const(256),
              "1 x 3000 then the rest": lambda call: 1 if call < 3000 else 1 << 30, "random 1..2000": lambda call: rng.randint(1, 2000)}
    got = {k: _stream_rows([x], [f], mean=mean, std=std)[0][0] for k, f in splits.items()}
    T = ops.n_frames(x.numel(), 1024, 256)
    assert T == 185
    for k, v in got.items():
        assert v.shape == (T, 513) and bool(torch.isfinite(v).all()), k
        assert torch.equal(v, got["one call"]), "split '%s' differs from one call: max|d| = %.3e" % (
            k, float((v - got["one call"]).abs().max()))


def test_row_and_batch_invariance_bit_for_bit():
    """The utterance as row 0 of B = 1 and as row 5 of B = 7 whose other rows carry other data, other packet sizes and
    other end times, one of them idle: the same bits; the idle row's state does not change."""
    x = _utt().to(DEV)
    mean, std = _stats()
    alone = _stream_rows([x], [_const(160)], mean=mean, std=std)[0][0]
    torch.manual_seed(3)
    rng = random.Random(9)
    others = [torch.randn(n, device=DEV) * s for n, s in ((30000, 0.1), (48100, 1.0), (700, 0.5), (51234, 0.02), (1024, 2.0))]
    rows = others[:2] + [None] + others[2:4] + [x] + others[4:]
    sizes = [_const(999), lambda c: rng.randint(0, 600), _const(0), _const(64), _const(4000), lambda c: rng.randint(1, 1500),
             _const(256)]
    from avvad import ops
    state = ops.stft_stream_state(7, 1024, DEV)
    state[2] = torch.randn(1024, device=DEV)                      # an idle row keeps whatever it holds
    idle = state[2].clone()
    outs, last, clock = _stream_rows(rows, sizes, mean=mean, std=std, state=state)
    assert torch.equal(outs[5], alone), "row 5 of 7 differs from row 0 of 1: max|d| = %.3e" % float((outs[5] - alone).abs().max())
    assert torch.equal(last[2], idle) and outs[2].shape[0] == 0 and clock.total[2] == 0
    for b, r in enumerate(rows):                                  # every other row against itself alone, too
        if r is not None and b != 5:
            assert torch.equal(outs[b], _stream_rows([r], [_const(333)], mean=mean, std=std)[0][0]), b


def test_state_in_place_equals_spare_and_peak_one_changes_no_bit():
    x = _utt().to(DEV)[:20000]
    y = torch.flip(x, [0]) * 0.5
    a, sa, _ = _stream_rows([x, y], [_const(160), _const(777)])
    b, sb, _ = _stream_rows([x, y], [_const(160), _const(777)], in_place=True)
    c, sc, _ = _stream_rows([x, y], [_const(160), _const(777)], peak=torch.ones(2, device=DEV))
    b2, sb2, _ = _stream_rows([x, y], [_const(160), _const(777)], in_place=True, name_state=True)      # out_state=state
    for r in range(2):
        assert torch.equal(a[r], b[r]) and torch.equal(a[r], b2[r]) and torch.equal(a[r], c[r])
    assert torch.equal(sa, sb) and torch.equal(sa, sb2) and torch.equal(sa, sc)
    from avvad import AvvadError, ops
    from avvad.stream import SampleClock
    ck = SampleClock(2, 1024, 256)
    with pytest.raises(AvvadError, match="out_state"):
        ops.stft_stream(torch.zeros(2, 160, device=DEV), None, ck, sa, ops.stft_stream_basis(1024, DEV), out_state=[1, 2])
    assert ck.total == [0, 0]
    d, _, _ = _stream_rows([x, y], [_const(160), _const(777)], peak=torch.tensor([2.0, 0.5], device=DEV))
    e, _, _ = _stream_rows([x / 2.0, y / 0.5], [_const(500), _const(100)])
    assert torch.equal(d[0], e[0]) and torch.equal(d[1], e[1])    # division by a power of two is exact: the same frames


def test_silence_gives_log_eps_exactly_where_the_whole_utterance_kernel_does():
    from avvad import ops
    x = _utt().to(DEV)[:12000].clone()
    x[2000:9000] = 0.0
    whole = ops.stft(x, 1024, 256, mode=0, eps=1e-8)[0]
    got = _stream_rows([x], [_const(160)])[0][0]
    assert got.shape == whole.shape
    log_eps = float(whole[12, 0])                                 # frames 8 .. 31 lie inside the zeros
    assert abs(log_eps - float(np.log(1e-8))) < 1e-5
    assert bool((whole[8:32] == log_eps).all()) and bool((got[8:32] == log_eps).all())
    assert torch.equal(got == log_eps, whole == log_eps)          # and nowhere else
    _report("features around a silence vs ops.stft", got, whole, 2e-3, 1e-4)


@pytest.mark.parametrize("n_fft,hop,with_stats", [(1024, 256, True), (1024, 256, False), (512, 128, False)])
def test_streamed_features_vs_oracle(n_fft, hop, with_stats):
    """utt_sa1 in 160-sample packets with the peak set to max|x| against the oracle's whole-utterance front-end."""
    from avvad import ops
    from oracle import frontend
    x = _utt()
    g = load_golden("eval_audio")
    n_label = int(g["n_label"])
    xd = x.to(DEV)
    peak = ops.peak(xd)
    assert float(peak[0]) == float(x.abs().max())
    mean, std = _stats() if with_stats else (None, None)
    got = _stream_rows([xd], [_const(160)], n_fft, hop, mean, std, peak)[0][0]
    if with_stats:
        ref = frontend.audio_features(x, T_(g["mean"]), T_(g["std"]), n_label)[0]
        got = got[:n_label]
    else:
        S = frontend.stft(x / x.abs().max(), wlen_sec=n_fft / 16e3, hop_percent=hop / n_fft, center=False, pad_at_end=True)
        ref = frontend.log_power(S).transpose(0, 1)
    assert got.shape[0] == ref.shape[0] or with_stats
    _report("streamed features n_fft %d %s vs oracle" % (n_fft, "standardised" if with_stats else "log-power"), got, ref,
            2e-3, 1e-4)


def _audio_model(tag, ydim):
    from packages.models.Audio_Net import DeepVAD_audio
    m = DeepVAD_audio(2, 32, ydim)
    m.load_state_dict(torch.load(os.path.join(GOLDEN, "audio_ref_h32_%s.pt" % tag), map_location="cpu", weights_only=True))
    return m.to(DEV).eval()


def _check_outputs(soft, hard, g, tag, name):
    _report(name + " soft output (%s)" % tag, soft, g["soft_" + tag], 1e-4)
    differ = hard.numpy() != g["hard_" + tag]
    margin = np.abs(g["soft_" + tag] - 0.5)
    assert int(differ.sum()) == 0 or float(margin[differ].max()) < 1e-4, int(differ.sum())


@pytest.mark.parametrize("tag,ydim", [("y1", 1), ("y513", 513)])
def test_evaluators_from_samples_on_a_real_utterance(tag, ydim, tmp_path):
    """process_utt(chunk_samples=160) and evaluate_main(chunk_samples=400) with the checkpoints the reference wrote, by
    the rule of test_audio_evaluator_plumbing_on_a_real_utterance."""
    from avvad import train as TR
    from packages.models.Audio_Net import DeepVAD_audio
    g = load_golden("eval_audio")
    wav = os.path.join(GOLDEN, "utt_sa1.npz")
    stats = TR.Stats(audio_mean=g["mean"], audio_std=g["std"])
    n_label = int(g["n_label"])
    soft, hard = TR.process_utt(_audio_model(tag, ydim), _utt().to(DEV), stats, n_label, chunk_samples=160)
    assert soft.shape == (1, n_label) and hard.dtype == torch.int32
    _check_outputs(soft, hard, g, tag, "process_utt(chunk_samples=160)")
    TR.evaluate_main("audio", lambda: DeepVAD_audio(2, 32, ydim), checkpoint=os.path.join(GOLDEN, "audio_ref_h32_%s.pt" % tag),
                     out_dir=str(tmp_path), wav_list=[wav], stats=stats, labels={wav: torch.zeros(ydim, n_label)},
                     chunk_samples=400)
    soft = torch.load(tmp_path / "utt_sa1_y_hat_soft.pt", weights_only=True)
    hard = torch.load(tmp_path / "utt_sa1_y_hat_hard.pt", weights_only=True)
    assert soft.shape == (1, n_label) and hard.dtype == torch.int32
    _check_outputs(soft, hard, g, tag, "evaluate_main(chunk_samples=400)")


def test_session_saved_mid_utterance_and_restored_continues_with_the_same_bits():
    from avvad import stream, train as TR
    g = load_golden("eval_audio")
    stats = TR.Stats(audio_mean=g["mean"], audio_std=g["std"])
    m = _audio_model("y1", 1)
    x = _utt().to(DEV).view(1, -1)
    a = stream.open(m, 1)
    a.set_frontend(stats)
    a.peak.fill_(float(x.abs().max()))
    first = []
    for s0 in range(0, 20000, 160):
        y, fr = a.step_wave(x[:, s0:s0 + 160].contiguous())
        first.append(y[:, :fr[0]])
    assert sum(t.shape[1] for t in first) == (20000 - 1024) // 256 + 1
    b = stream.open(m, 1)
    b.set_frontend(stats)
    b.prepare_frontend()                                          # the front-end state exists before it is restored
    ck, ca = b.sample_clock, a.sample_clock
    b.h.copy_(a.h), b.c.copy_(a.c), b.stft_state.copy_(a.stft_state), b.peak.copy_(a.peak)
    ck.total, ck.emitted, ck.pending, ck.ended = list(ca.total), list(ca.emitted), list(ca.pending), list(ca.ended)
    rest_a, rest_b = [], []
    for s0 in range(20000, x.shape[1], 160):                     # the original and the restored session take the same packets
        y, fr = a.step_wave(x[:, s0:s0 + 160].contiguous(), final=[0] if s0 + 160 >= x.shape[1] else None)
        rest_a.append(y[:, :fr[0]])
    for s0 in range(20000, x.shape[1], 160):
        y, fr = b.step_wave(x[:, s0:s0 + 160].contiguous(), final=[0] if s0 + 160 >= x.shape[1] else None)
        rest_b.append(y[:, :fr[0]])
    ya, yb = torch.cat(first + rest_a, 1), torch.cat(first + rest_b, 1)
    assert ya.shape == (1, 185, 1)
    assert torch.equal(torch.cat(rest_a, 1), torch.cat(rest_b, 1))
    soft = torch.sigmoid(ya[..., 0].cpu())[:, :int(g["n_label"])]
    _report("session from samples, soft output (y1)", soft, g["soft_y1"], 1e-4)
    a.reset([0])                                                  # the peak goes back to 1, the front-end starts over
    assert float(a.peak[0]) == 1.0 and a.sample_clock.total == [0] and float(a.stft_state.abs().max()) == 0.0
    y, fr = a.step_wave(x[:, :1023].contiguous())
    assert y.shape == (1, 0, 1) and fr == [0]


def test_step_wave_checks_before_it_changes_anything():
    from avvad import AvvadError, stream
    m = _audio_model("y1", 1)
    s = stream.open(m, 2)
    w = torch.randn(2, 1500, device=DEV)
    s.step_wave(w, samples=[1500, 700])
    before = (s.h.clone(), s.c.clone(), s.stft_state.clone(), list(s.sample_clock.total), list(s.sample_clock.pending))
    for bad in (dict(wave=w.cpu()), dict(wave=w.double()), dict(wave=w[:1]), dict(wave=w, samples=[1, 2, 3]),
                dict(wave=w, samples=[1501, 0]), dict(wave=w, samples=[-1, 0]), dict(wave=w, final=[2]),
                dict(wave=w, video=torch.zeros(2, 1, 67, 67, device=DEV))):
        with pytest.raises(AvvadError):
            s.step_wave(**bad)
        assert torch.equal(s.h, before[0]) and torch.equal(s.c, before[1]) and torch.equal(s.stft_state, before[2])
        assert s.sample_clock.total == before[3] and s.sample_clock.pending == before[4]
    s.step_wave(w[:, :10].contiguous(), final=[1])
    with pytest.raises(AvvadError, match="reset"):
        s.step_wave(w[:, :10].contiguous())                       # row 1 ended
    s.reset([1])
    s.step_wave(w[:, :10].contiguous())
    from packages.models.Video_Net import DeepVAD_video
    with pytest.raises(AvvadError, match="step_wave"):
        stream.open(DeepVAD_video(1, 16, 1).to(DEV).eval(), 1).step_wave(w[:1])


def test_av_concat_step_wave_vs_whole_utterance_forward():
    """DeepVAD_AV (concat fusion, random weights) on two ragged rows: samples and lip frames through step_wave against
    model.eval()(ops.stft features, video, lengths)."""
    from avvad import ops, stream
    from packages.models.AV_Net import DeepVAD_AV
    torch.manual_seed(21)
    m = DeepVAD_AV(2, 32, 1).to(DEV).eval()
    lens = [5000, 3100]
    w = torch.randn(2, 5000, device=DEV) * 0.3
    w[1, 3100:] = 0.0
    T = [ops.n_frames(n, 1024, 256) for n in lens]
    assert T == [17, 10]
    video = torch.randn(2, T[0], 67, 67, device=DEV)
    feats = torch.zeros(2, T[0], 513, device=DEV)
    for b in range(2):
        feats[b, :T[b]] = ops.stft(w[b, :lens[b]].contiguous(), 1024, 256, mode=0)[0]
    with torch.no_grad():
        ref = m(feats, video, T)
    y = stream.forward_wave_chunked(m, w, lens, video, 700)
    assert y.shape == ref.shape
    for b in range(2):
        _report("DeepVAD_AV concat from samples, row %d" % b, y[b, :T[b]], ref[b, :T[b]], 1e-4)
    # by hand: the caller asks the clock how many lip frames the next samples need
    s = stream.open(m, 2)
    done, outs = [0, 0], [[], []]
    for s0 in range(0, 5000, 900):
        n = [min(max(l - s0, 0), 900) for l in lens]
        fin = [b for b in range(2) if 0 < lens[b] - s0 <= 900]
        frames = s.sample_clock.plan(n, fin)
        v = torch.zeros(2, max(frames), 67, 67, device=DEV)
        for b in range(2):
            v[b, :frames[b]] = video[b, done[b]:done[b] + frames[b]]
        yy, fr = s.step_wave(w[:, s0:s0 + 900].contiguous(), n, v if max(frames) else None, fin)
        assert fr == frames
        for b in range(2):
            outs[b].append(yy[b, :fr[b]])
            done[b] += fr[b]
    assert done == T
    for b in range(2):
        _report("DeepVAD_AV concat from samples by hand, row %d" % b, torch.cat(outs[b], 0), ref[b, :T[b]], 1e-4)


def test_av_evaluator_from_samples_writes_what_the_whole_utterance_route_writes(tmp_path):
    """evaluate_main(av_files=..., chunk_samples=) against the same call without it: the same model (seeded in
    evaluate_main), the same files, soft outputs within the project's output bound and labels identical."""
    from avvad import train as TR
    from packages.models.AV_Net import DeepVAD_AV
    from test_lip_gpu import av_fixture
    triples, listing = av_fixture(tmp_path)
    outs = {}
    for name, kw in (("whole", {}), ("samples", dict(chunk_samples=400))):
        outs[name] = str(tmp_path / ("eval_" + name))
        TR.evaluate_main("AV", lambda: DeepVAD_AV(1, 16, 1), out_dir=outs[name], av_files=listing, **kw)
    files = sorted(f for f in os.listdir(outs["whole"]) if f.endswith(".pt"))
    assert len(files) == 3 * len(triples) and files == sorted(f for f in os.listdir(outs["samples"]) if f.endswith(".pt"))
    for f in files:
        a = torch.load(os.path.join(outs["whole"], f), weights_only=True)
        b = torch.load(os.path.join(outs["samples"], f), weights_only=True)
        if f.endswith("_y_hat_soft.pt"):
            _report("AV evaluator from samples, " + f, b, a, 1e-4)
        elif f.endswith("_label.pt"):
            assert torch.equal(a, b), f
        else:
            soft = torch.load(os.path.join(outs["whole"], f.replace("_hard", "_soft")), weights_only=True)
            differ = a != b
            assert int(differ.sum()) == 0 or float((soft - 0.5).abs()[differ].max()) < 1e-4, f


@pytest.mark.parametrize("n_fft", [32, 64])
def test_streaming_basis_is_the_whole_utterance_basis(n_fft):
    """Frame t of the wave is a unit impulse at sample t, so the whole-utterance DFT returns its basis exactly (one
    non-zero product per sum); the streaming kernel's packed basis must hold the same floats, and zeros for the bins of
    its last 16-bin block that lie at or beyond F."""
    from avvad import ops
    N, F = n_fft, n_fft // 2 + 1
    wave = torch.zeros(1, N * N, device=DEV)
    wave[0, torch.arange(N, device=DEV) * (N + 1)] = 1.0
    whole = ops.stft_complex(wave, N, N, pad_at_end=False)[0].cpu()                  # [k][f][re, im]
    assert whole.shape == (N, F, 2)
    blocks = (F + 15) // 16
    packed = ops.stft_stream_basis(N, DEV).cpu().view(blocks, 2, N // 16, 64, 4)     # [bin block][re, im][kk][lane][j]
    lane = torch.arange(64).view(1, 64, 1)
    k = (N // 4) * (lane >> 4) + 4 * torch.arange(N // 16).view(-1, 1, 1) + torch.arange(4).view(1, 1, 4)
    for b in range(blocks):
        f = (16 * b + (lane & 15)).expand_as(k)
        inside = f < F
        for c in range(2):
            want = torch.zeros(N // 16, 64, 4)
            want[inside] = whole[k[inside], f[inside], c]
            assert bool((packed[b, c] == want).all()), (b, c)
            assert not packed[b, c][~inside].any()
    assert blocks * 16 > F                                                           # the last block is partly beyond F
