"""Streaming inference on the GPU: the LSTM layer with state, the streaming encoder and the session, against torch on
the CPU, the oracle and the golden vectors the reference produced.  Bounds are the project's own: outputs |d| <= 1e-4
(BASELINE north star); intermediate / unbounded quantities (c_n) atol 1e-4 + rtol 1e-5 |ref|, as on the trunk
features.  Observed maxima are appended to the parity log, the way test_gpu_parity._report does.  The kernels themselves,
fed directly with per-row schedules and held element-wise to float64 references, are in tests/test_stream_kernels_gpu.py
(oracle: tests/stream_ref.py)."""
import os
import random

import numpy as np
import pytest
import torch

import stategen
from conftest import GOLDEN, load_golden, wn_cfg_from

from test_gpu_parity import OUT, _report as _parity_report

pytestmark = pytest.mark.gpu
T_ = torch.from_numpy
DEV = "cuda:0"


def _report(name, got, ref, atol, rtol=0.0):
    """The parity suite's own report: prints the observed maximum, appends it to the parity log, then asserts."""
    _parity_report("stream: " + name, got, ref, atol, rtol)


def _ragged(rng, B, T):
    """lengths in [0, T] that contain a 0 (when B > 1) and a T"""
    lens = [rng.randint(0, T) for _ in range(B)]
    lens[0] = T
    if B > 1:
        lens[-1] = 0
    return lens


# ------------------------------------------------------------------------------------------ LSTM layer with state
def _torch_lstm_rows(lstm, x, lens, h0, c0):
    """torch.nn.LSTM on the CPU, row by row (a packed batch cannot hold a length 0)."""
    B, T, _ = x.shape
    y = torch.zeros(B, T, lstm.hidden_size)
    hn, cn = h0.clone(), c0.clone()
    with torch.no_grad():
        for b, n in enumerate(lens):
            if n == 0:
                continue
            o, (h, c) = lstm(x[b:b + 1, :n].transpose(0, 1).contiguous(), (h0[:, b:b + 1].contiguous(), c0[:, b:b + 1].contiguous()))
            y[b, :n] = o[:, 0]
            hn[:, b], cn[:, b] = h[:, 0], c[:, 0]
    return y, hn, cn


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("In", [40, 513, 1025])
@pytest.mark.parametrize("H", [64, 1024])
@pytest.mark.parametrize("B", [1, 3, 16, 17, 64])
def test_lstm_state_vs_torch(B, H, In, T):
    """ops.lstm_stack_state against torch.nn.LSTM on the CPU from random non-zero (h0, c0): y, h_n, c_n; ragged lengths
    with a 0; a length-0 row keeps its state bit for bit; writing the state in place gives the same bits."""
    from avvad import ops
    torch.manual_seed(B * 7919 + H + In + T)
    rng = random.Random(B + H + In + T)
    lstm = torch.nn.LSTM(In, H, 2)
    x = torch.randn(B, T, In)
    h0, c0 = torch.randn(2, B, H) * 0.5, torch.randn(2, B, H)
    lens = _ragged(rng, B, T)
    ry, rh, rc = _torch_lstm_rows(lstm, x, lens, h0, c0)
    g = lstm.to(DEV)
    hd, cd = h0.to(DEV), c0.to(DEV)
    y, (hn, cn) = ops.lstm_stack_state(x.to(DEV), lens, g, state=(hd, cd))
    tag = "B%d H%d In%d T%d" % (B, H, In, T)
    _report("lstm_stack_state y vs torch.nn.LSTM " + tag, y, ry, 1e-4)
    _report("lstm_stack_state h_n vs torch.nn.LSTM " + tag, hn, rh, 1e-4)
    _report("lstm_stack_state c_n vs torch.nn.LSTM " + tag, cn, rc, 1e-4, 1e-5)
    assert torch.equal(hd.cpu(), h0) and torch.equal(cd.cpu(), c0)            # inputs untouched when out is separate
    for b, n in enumerate(lens):
        if n == 0:
            assert torch.equal(hn[:, b].cpu(), h0[:, b]) and torch.equal(cn[:, b].cpu(), c0[:, b]), "row %d" % b
            assert float(y[b].abs().max()) == 0.0
    y2, (h2, c2) = ops.lstm_stack_state(x.to(DEV), lens, g, state=(hd, cd), out=(hd, cd))
    assert h2 is hd and c2 is cd
    assert torch.equal(y2, y) and torch.equal(hd, hn) and torch.equal(cd, cn)
    y3, (h3, c3) = ops.lstm_stack_state(x.to(DEV), lens, g)                    # state=None means zeros
    y4, (h4, c4) = ops.lstm_stack_state(x.to(DEV), lens, g, state=(torch.zeros_like(hd), torch.zeros_like(cd)))
    assert torch.equal(y3, y4) and torch.equal(h3, h4) and torch.equal(c3, c4)


def test_lstm_state_odd_hidden_size():
    """H % 4 != 0 (scalar loads, a workgroup with surplus units) and B > 64 (several column runs)."""
    from avvad import ops
    torch.manual_seed(3)
    B, T, In, H = 70, 3, 9, 50
    lstm = torch.nn.LSTM(In, H, 2)
    x, h0, c0 = torch.randn(B, T, In), torch.randn(2, B, H) * 0.5, torch.randn(2, B, H)
    lens = _ragged(random.Random(5), B, T)
    ry, rh, rc = _torch_lstm_rows(lstm, x, lens, h0, c0)
    y, (hn, cn) = ops.lstm_stack_state(x.to(DEV), lens, lstm.to(DEV), state=(h0.to(DEV), c0.to(DEV)))
    _report("lstm_stack_state y vs torch.nn.LSTM B70 H50", y, ry, 1e-4)
    _report("lstm_stack_state h_n vs torch.nn.LSTM B70 H50", hn, rh, 1e-4)
    _report("lstm_stack_state c_n vs torch.nn.LSTM B70 H50", cn, rc, 1e-4, 1e-5)


def test_lstm_chunk_invariance_vs_oracle():
    """A 2 x 1024 stack over a ragged batch, split as [1]*T, [T] and a random split, each against the oracle's
    whole-sequence head.lstm_stack."""
    from avvad import ops
    from oracle import head
    B, T, In, H = 5, 12, 513, 1024
    sd = stategen.make_state(stategen.lstm_spec("lstm_audio.", In, H, 2), 31)
    x = stategen.rand(32, B, T, In)
    lens = [12, 7, 1, 0, 9]
    ref = head.lstm_stack(x, lens, sd, "lstm_audio.", 2)
    lstm = torch.nn.LSTM(In, H, 2)
    lstm.load_state_dict({k[len("lstm_audio."):]: v for k, v in sd.items()})
    lstm = lstm.to(DEV)
    rng = random.Random(9)
    cuts = []
    while sum(cuts) < T:
        cuts.append(min(rng.randint(1, 5), T - sum(cuts)))
    xd = x.to(DEV)
    for name, split in (("[1]*T", [1] * T), ("[T]", [T]), ("random %s" % cuts, cuts)):
        state, outs, t0 = None, [], 0
        for n in split:
            ln = [min(max(l - t0, 0), n) for l in lens]
            y, state = ops.lstm_stack_state(xd[:, t0:t0 + n].contiguous(), ln, lstm, state=state)
            outs.append(y)
            t0 += n
        _report("2x1024 LSTM chunks %s vs oracle whole sequence" % name, torch.cat(outs, 1), ref, 1e-4)


# ------------------------------------------------------------------------------------------ the reference's own outputs
def _stream_all(sess, T, chunk, lens, audio=None, video=None):
    outs = []
    for t0 in range(0, T, chunk):
        t1 = min(t0 + chunk, T)
        ln = [min(max(l - t0, 0), t1 - t0) for l in lens]
        outs.append(sess.step(audio[:, t0:t1].contiguous() if audio is not None else None,
                              video[:, t0:t1].contiguous() if video is not None else None, ln))
    return torch.cat(outs, 1)


def test_audio_golden_streamed():
    from avvad import stream
    from packages.models.Audio_Net import DeepVAD_audio
    g = load_golden("audio_l2_h16")
    Ln, H, ydim = [int(v) for v in g["meta"]]
    m = DeepVAD_audio(Ln, H, ydim)
    m.load_state_dict(stategen.make_state(stategen.lstm_spec("lstm_audio.", 513, H, Ln) +
                                          stategen.linear_spec("vad_audio", H, ydim), 1))
    m = m.to(DEV).eval()
    lens = g["lengths"].tolist()
    assert lens == [7, 5, 2]
    y = _stream_all(stream.open(m, 3), 7, 2, lens, audio=T_(g["x"]).to(DEV))
    _report("audio_l2_h16 streamed in chunks of 2 vs the reference's y", y, g["y"], 1e-4)


def test_video_golden_streamed():
    from avvad import stream
    from oracle import resnet18
    from packages.models.Video_Net import DeepVAD_video
    g = load_golden("video_h16")
    m = DeepVAD_video(2, 16, 1)
    m.load_state_dict(stategen.make_state(resnet18.trunk_keys("features.") + stategen.lstm_spec("lstm_video.", 512, 16, 2) +
                                          stategen.linear_spec("vad_video", 16, 1), 7))
    m = m.to(DEV).eval()
    x = T_(g["x"]).to(DEV)
    y = _stream_all(stream.open(m, x.shape[0]), x.shape[1], 1, g["lengths"].tolist(), video=x)
    _report("video_h16 streamed one frame per step vs the reference's y_eval", y, g["y_eval"], 1e-4)


def test_av_concat_golden_streamed():
    from avvad import stream
    from packages.models.AV_Net import DeepVAD_AV
    g = load_golden("av_concat_h16")
    keys = [str(k) for k in g["keys"]]
    shapes = [eval(str(s)) for s in g["shapes"]]
    m = DeepVAD_AV(2, 16, 1)
    m.load_state_dict(stategen.make_state(list(zip(keys, shapes)), 11))
    m = m.to(DEV).eval()
    a, v = T_(g["audio"]).to(DEV), T_(g["video"]).to(DEV)
    y = _stream_all(stream.open(m, a.shape[0]), a.shape[1], 1, g["lengths"].tolist(), audio=a, video=v)
    _report("av_concat_h16 streamed one frame per step vs the reference's y_eval", y, g["y_eval"], 1e-4)


@pytest.mark.parametrize("c", [1, 7])
def test_evaluator_in_chunks_on_a_real_utterance(c, tmp_path):
    """evaluate_main(..., chunk_frames=c) on utt_sa1 with the checkpoint the reference wrote, by the criterion of
    test_audio_evaluator_plumbing_on_a_real_utterance: soft within 1e-4, a hard flip only where the reference's margin is
    below 1e-4."""
    from avvad import train as TR
    from packages.models.Audio_Net import DeepVAD_audio
    g = load_golden("eval_audio")
    wav = os.path.join(GOLDEN, "utt_sa1.npz")
    stats = TR.Stats(audio_mean=g["mean"], audio_std=g["std"])
    n_label = int(g["n_label"])
    assert n_label == 180
    TR.evaluate_main("audio", lambda: DeepVAD_audio(2, 32, 1), checkpoint=os.path.join(GOLDEN, "audio_ref_h32_y1.pt"),
                     out_dir=str(tmp_path), wav_list=[wav], stats=stats, labels={wav: torch.zeros(1, n_label)},
                     chunk_frames=c)
    soft = torch.load(tmp_path / "utt_sa1_y_hat_soft.pt", weights_only=True)
    hard = torch.load(tmp_path / "utt_sa1_y_hat_hard.pt", weights_only=True)
    assert soft.shape == (1, n_label) and hard.dtype == torch.int32
    _report("evaluate_main(chunk_frames=%d) soft vs the reference's soft_y1" % c, soft, g["soft_y1"], 1e-4)
    diff = hard.numpy() != g["hard_y1"]
    margin = np.abs(g["soft_y1"] - 0.5)
    assert int(diff.sum()) == 0 or float(margin[diff].max()) < 1e-4, int(diff.sum())


# ------------------------------------------------------------------------------------------ encoder
def _encoder_from_golden(g):
    from packages.models.wavenet_autoencoder import wavenet_autoencoder
    m = wavenet_autoencoder(**wn_cfg_from(g))
    m.load_state_dict({k[2:]: T_(v) for k, v in g.items() if k.startswith("p.")})
    return m.to(DEV).eval()


def _stream_encoder(enc, x, k, cuts):
    """x (B,qc,L) on the GPU cut at the sample positions `cuts` (per call, the same for every row) -> (B, frames, Bn)"""
    from avvad import ops
    from avvad.stream import FrameClock
    B = x.shape[0]
    clock = FrameClock(B, enc.receptive_field, k)
    state = ops.wavenet_stream_state(enc, B, x.device)
    outs, s0 = [], 0
    for n in cuts:
        frames, used = clock.advance([n] * B)
        outs.append(ops.wavenet_stream(x[:, :, s0:s0 + n].contiguous(), [n] * B, used, enc, state, k, max(frames)))
        s0 += n
    assert s0 == x.shape[2]
    return torch.cat(outs, 1)


def test_encoder_w0_golden_streamed():
    """wn_w0_t16: valid length 4096, P = 16, so k = 256; the reference's y is (B, Bn, P)."""
    g = load_golden("wn_w0_t16")
    enc = _encoder_from_golden(g)
    x = T_(g["x"]).to(DEV)
    ref = T_(g["y"]).permute(0, 2, 1)
    assert enc.receptive_field == 2048 and x.shape[2] == 2047 + 16 * 256
    even = [2047 + 256] + [256] * 15
    uneven = [1000, 1047, 256 * 3, 256, 256 * 7, 256 * 5]
    whole = [x.shape[2]]
    for name, cuts in (("even", even), ("uneven, warm-up in two calls", uneven), ("one call", whole)):
        _report("wn_w0_t16 streamed (%s) vs the reference's y" % name, _stream_encoder(enc, x, 256, cuts), ref, 1e-4)


def test_encoder_nobias_golden_streamed():
    """wn_nobias: valid length 284, P = 4, so k = 71."""
    g = load_golden("wn_nobias")
    enc = _encoder_from_golden(g)
    x = T_(g["x"]).to(DEV)
    ref = T_(g["y"]).permute(0, 2, 1)
    assert x.shape[2] == enc.receptive_field - 1 + 4 * 71
    for name, cuts in (("even", [16 + 71, 71, 71, 71]), ("uneven", [5, 11 + 142, 142]), ("one call", [300])):
        _report("wn_nobias streamed (%s) vs the reference's y" % name, _stream_encoder(enc, x, 71, cuts), ref, 1e-4)


@pytest.mark.parametrize("name,P,k", [("wn_fw3_qc2", 5, 9), ("wn_tiny", 6, 40), ("wn_tiny", 3, 300)])
def test_encoder_direct_form_vs_oracle(name, P, k):
    """The plain direct form (fw = 3 / qc = 2, and R = D = 4) against oracle.wavenet.encode on L = RF-1 + P*k samples,
    where the adaptive pool has uniform windows of k; k = 300 makes a frame straddle two passes of the kernel."""
    from oracle import wavenet
    from packages.models.wavenet_autoencoder import wavenet_autoencoder
    cfg = dict(wn_cfg_from(load_golden(name)), en_pool_kernel_size=P)
    sd = stategen.make_state(stategen.wavenet_spec(cfg), 41)
    rf = wavenet.receptive_field(cfg["filter_width"], cfg["dilations"])
    B, Ln = 3, rf - 1 + P * k
    x = stategen.rand(42, B, cfg["quantization_channel"], Ln, scale=0.5)
    ref = wavenet.encode(sd, x, cfg).permute(0, 2, 1)
    enc = wavenet_autoencoder(**cfg)
    enc.load_state_dict(sd)
    enc = enc.to(DEV).eval()
    rng = random.Random(k)
    cuts = [rng.randint(1, rf - 1) if rf > 2 else rf - 1]
    cuts.append(rf - 1 - cuts[0] + k)
    left = P - 1
    while left:
        f = rng.randint(1, left)
        cuts.append(f * k)
        left -= f
    cuts = [c for c in cuts if c > 0]
    for nm, cc in (("random cuts %s" % cuts, cuts), ("one call", [Ln])):
        _report("%s P=%d k=%d streamed (%s) vs oracle.wavenet.encode" % (name, P, k, nm),
                _stream_encoder(enc, x.to(DEV), k, cc), ref, 1e-4)


# ------------------------------------------------------------------------------------------ end to end
WCFG = dict(filter_width=2, quantization_channel=1, dilations=[1, 2, 4, 8, 16, 32], en_residual_channel=32,
            en_dilation_channel=32, en_bottleneck_width=64, en_pool_kernel_size=4, use_bias=True)


def _av_model(seed):
    from packages.models.AV_Net import DeepVAD_AV
    torch.manual_seed(seed)
    m = DeepVAD_AV(2, 32, 1, wavenet_params=WCFG)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.to(DEV).eval(), sd


def test_av_with_encoder_end_to_end_with_a_reset():
    """DeepVAD_AV with the encoder in chunks against oracle.models.av_net(training=False): row 1 is reset mid-way and
    starts a second utterance; both utterances must match their own whole-utterance reference."""
    from avvad import stream
    from oracle import models
    m, sd = _av_model(5)
    rf, k = 65, 256                                 # 1 + sum of the dilations
    T1, T2 = 4, 2                                   # row 0: one utterance of 6 frames; row 1: 4 frames, reset, 2 frames
    torch.manual_seed(6)
    w0, v0 = torch.randn(1, 1, rf - 1 + 6 * k) * 0.3, torch.randn(1, 6, 67, 67)
    w1a, v1a = torch.randn(1, 1, rf - 1 + T1 * k) * 0.3, torch.randn(1, T1, 67, 67)
    w1b, v1b = torch.randn(1, 1, rf - 1 + T2 * k) * 0.3, torch.randn(1, T2, 67, 67)
    ref0 = models.av_net(sd, w0, v0, [6], 2, training=False, wavenet_cfg=dict(WCFG, en_pool_kernel_size=6))
    ref1a = models.av_net(sd, w1a, v1a, [T1], 2, training=False, wavenet_cfg=dict(WCFG, en_pool_kernel_size=T1))
    ref1b = models.av_net(sd, w1b, v1b, [T2], 2, training=False, wavenet_cfg=dict(WCFG, en_pool_kernel_size=T2))
    sess = stream.open(m, 2, samples_per_frame=k)
    warm = rf - 1

    def call(a0, a1, f0, f1):
        """feed row 0 the samples a0 of w0 / frames f0 of v0, row 1 likewise from its current utterance"""
        n = [a0.shape[2], a1.shape[2]]
        L = max(n)
        audio = torch.zeros(2, 1, L)
        audio[0, :, :n[0]], audio[1, :, :n[1]] = a0[0], a1[0]
        tl = max(f0.shape[1], f1.shape[1])
        video = torch.zeros(2, tl, 67, 67)
        video[0, :f0.shape[1]], video[1, :f1.shape[1]] = f0[0], f1[0]
        return sess.step(audio.to(DEV), video.to(DEV), [f0.shape[1], f1.shape[1]], samples=n)

    # step 1: row 0 warm-up + 2 frames, row 1 warm-up + 1 frame
    y = call(w0[:, :, :warm + 2 * k], w1a[:, :, :warm + k], v0[:, :2], v1a[:, :1])
    o0, o1a = [y[0:1, :2]], [y[1:2, :1]]
    # step 2: row 0 one frame, row 1 three frames (ends its first utterance)
    y = call(w0[:, :, warm + 2 * k:warm + 3 * k], w1a[:, :, warm + k:], v0[:, 2:3], v1a[:, 1:])
    o0.append(y[0:1, :1]); o1a.append(y[1:2, :3])
    sess.reset([1])
    assert sess.clock.skip == [0, warm]
    # step 3: row 0 two frames; row 1 only part of its new warm-up (no frame)
    y = call(w0[:, :, warm + 3 * k:warm + 5 * k], w1b[:, :, :20], v0[:, 3:5], v1b[:, :0])
    o0.append(y[0:1, :2])
    # step 4: row 0 the last frame; row 1 the rest of the warm-up and both frames
    y = call(w0[:, :, warm + 5 * k:], w1b[:, :, 20:], v0[:, 5:], v1b)
    o0.append(y[0:1, :1])
    _report("AV+encoder session row 0 (6 frames in 4 steps) vs oracle av_net", torch.cat(o0, 1), ref0, 1e-4)
    _report("AV+encoder session row 1 first utterance vs oracle av_net", torch.cat(o1a, 1), ref1a, 1e-4)
    _report("AV+encoder session row 1 after reset vs oracle av_net", y[1:2, :2], ref1b, 1e-4)
    from avvad import AvvadError
    before = (list(sess.clock.skip), sess.enc_state.clone(), sess.h.clone())
    with pytest.raises(AvvadError, match="H, W"):
        sess.step(torch.zeros(2, 1, k, device=DEV), torch.zeros(2, 1, 5, 5, device=DEV))          # frames agree, size does not
    assert sess.clock.skip == before[0] and torch.equal(sess.enc_state, before[1]) and torch.equal(sess.h, before[2])
    with pytest.raises(AvvadError, match="frames"):
        sess.step(torch.zeros(2, 1, k, device=DEV), torch.zeros(2, 2, 67, 67, device=DEV))       # audio: 1 frame, video: 2


def test_forward_chunked_waveform_model_vs_whole_forward():
    """forward_chunked on a ragged waveform batch equals the model's own whole-length eval forward at every valid frame."""
    from avvad import stream
    m, _ = _av_model(8)
    rf, k, T = 65, 256, 5
    torch.manual_seed(9)
    wave = (torch.randn(3, 1, rf - 1 + T * k) * 0.3).to(DEV)
    video = torch.randn(3, T, 67, 67).to(DEV)
    lens = [5, 3, 1]
    m.wavenet_en.en_pool_kernel_size = T
    with torch.no_grad():
        whole = m(wave, video, lens)
    y = stream.forward_chunked(m, wave, video, lens, chunk_frames=2, samples_per_frame=k)
    assert y.shape == whole.shape
    for b, n in enumerate(lens):
        _report("forward_chunked row %d vs the whole-length forward" % b, y[b, :n], whole[b, :n], 1e-4)


# ------------------------------------------------------------------------------------------ isolation and determinism
def _session_script(m, wave, video, perturb=None):
    """one fixed session script over 3 rows; `perturb` changes rows 1 and 2 only (inputs and states)"""
    from avvad import stream
    rf, k = 65, 256
    sess = stream.open(m, 3, samples_per_frame=k)
    warm = rf - 1
    if perturb is not None:
        wave, video = wave.clone(), video.clone()
        wave[1:] += perturb
        video[1:] -= perturb
    outs = []
    y = sess.step(wave[:, :, :warm + k].contiguous(), video[:, :1].contiguous())
    outs.append(y)
    if perturb is not None:
        sess.h[:, 1:] += perturb
        sess.c[:, 1:] -= perturb
        sess.enc_state[1:, 4:] += perturb
    y = sess.step(wave[:, :, warm + k:warm + 3 * k].contiguous(), video[:, 1:3].contiguous(), [2, 2, 1],
                  samples=[2 * k, 2 * k, k])
    outs.append(y)
    y = sess.step(wave[:, :, warm + 3 * k:warm + 4 * k].contiguous(), video[:, 3:4].contiguous(), [1, 0, 1], samples=[k, 0, k])
    outs.append(y)
    return torch.cat(outs, 1), sess


def test_rows_are_isolated_and_runs_are_bit_identical():
    m, _ = _av_model(12)
    torch.manual_seed(13)
    wave = (torch.randn(3, 1, 64 + 4 * 256) * 0.3).to(DEV)
    video = torch.randn(3, 4, 67, 67).to(DEV)
    y1, s1 = _session_script(m, wave, video)
    y2, s2 = _session_script(m, wave, video)
    assert torch.equal(y1, y2) and torch.equal(s1.h, s2.h) and torch.equal(s1.c, s2.c) and torch.equal(s1.enc_state, s2.enc_state)
    y3, s3 = _session_script(m, wave, video, perturb=0.25)
    assert torch.equal(y1[0], y3[0]), "row 0 changed when only the other rows' inputs and states did"
    assert torch.equal(s1.h[:, 0], s3.h[:, 0]) and torch.equal(s1.c[:, 0], s3.c[:, 0])
    assert torch.equal(s1.enc_state[0], s3.enc_state[0])
    assert not torch.equal(y1[1:], y3[1:])
    with open(os.path.join(OUT, "parity.log"), "a") as f:
        f.write("stream: session script twice: outputs and states bit-identical; row 0 bit-identical under changes to rows 1-2\n")
