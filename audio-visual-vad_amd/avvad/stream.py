"""Streaming inference: feed a model the next few frames, get the logits of exactly those frames.

``open(model, batch)`` returns a :class:`Session` that holds the state of ``batch`` independent streams ("rows") of one
model in ``eval()`` mode: the LSTM state (h, c) and, when the model carries the WaveNet encoder, every encoder layer's
left context.  The architecture is causal end to end -- the encoder is a valid (left-context-only) dilated Conv1d stack,
the ResNet trunk and the concat fusion are per frame, the LSTMs are unidirectional -- so the outputs of any split of an
utterance into chunks, concatenated, equal ``model.eval()(whole utterance)`` at every valid frame, and the cost of a
decision does not grow with the position in the utterance.

What stays OUTSIDE a session: statistics over the whole utterance.  Peak normalisation of a waveform
(``ops.peak_normalize``) and the lip decoder's min / max (``ops.lip_decode``) need all of it; a session takes features,
frames or samples that are already scaled.

``DeepVAD_AV(use_mcb=True)`` is refused: the reference divides the fused tensor by the L2 norm of the WHOLE (B, T, 1024)
tensor (``AV_Net.py:117``), which is neither causal nor per row, so no chunked evaluation can equal it.
"""
import torch

from . import _lib as L
from . import nn as avnn
from . import ops


class FrameClock:
    """Host-side bookkeeping of the encoder's warm-up and frame count, per row (resets come from the host, so this
    lives there too).  After a reset a row's first ``receptive_field - 1`` samples produce no frame; ``skip[b]`` is
    what is left of that.  A call with ``n_b`` real samples for row b is legal when ``n_b <= skip[b]`` (still warming
    up: no frame) or ``(n_b - skip[b]) % samples_per_frame == 0`` (whole frames only, none straddles two calls)."""

    def __init__(self, batch, receptive_field, samples_per_frame=256):
        if batch < 1 or samples_per_frame < 1 or receptive_field < 1:
            raise L.AvvadError("FrameClock needs batch, samples_per_frame and receptive_field >= 1")
        self.k = int(samples_per_frame)
        self.warmup = int(receptive_field) - 1
        self.skip = [self.warmup] * int(batch)

    def reset(self, rows=None):
        for b in (range(len(self.skip)) if rows is None else rows):
            self.skip[b] = self.warmup

    def plan(self, n):
        """Frames each row yields from ``n[b]`` samples; raises :class:`AvvadError` when a row breaks the rule.
        Changes nothing."""
        if len(n) != len(self.skip):
            raise L.AvvadError("one sample count per row expected (%d), got %d" % (len(self.skip), len(n)))
        frames = []
        for b, (nb, sb) in enumerate(zip(n, self.skip)):
            nb = int(nb)
            if nb < 0:
                raise L.AvvadError("row %d: negative sample count" % b)
            if nb <= sb:
                frames.append(0)
            elif (nb - sb) % self.k:
                raise L.AvvadError("row %d: %d samples after %d of warm-up leave %d over whole frames of %d: a frame may "
                                   "not straddle two calls" % (b, nb, sb, (nb - sb) % self.k, self.k))
            else:
                frames.append((nb - sb) // self.k)
        return frames

    def advance(self, n):
        """``plan`` and then consume: -> (frames per row, the skip counts that applied to THIS call)."""
        frames = self.plan(n)
        used = list(self.skip)
        self.skip = [max(sb - int(nb), 0) for nb, sb in zip(n, self.skip)]
        return frames, used


def _int_list(v, B, what, hi):
    if v is None:
        return [hi] * B
    v = [int(x) for x in (v.tolist() if isinstance(v, torch.Tensor) else v)]
    if len(v) != B or any(x < 0 or x > hi for x in v):
        raise L.AvvadError("%s must hold one value in [0, %d] per row (%d rows), got %s" % (what, hi, B, v))
    return v


class Session:
    """State of ``batch`` streams of one model.  Attributes a caller may save, restore or move between sessions:
    ``h`` / ``c`` (num_layers, batch, H) LSTM state, ``enc_state`` (batch, floats) encoder state (None without an
    encoder; all zeros = start of utterance) and ``clock.skip`` (host list: remaining warm-up samples per row).  A step
    writes the new LSTM state into a spare pair of tensors and swaps, so read ``h`` / ``c`` from the session after each
    step, not from a reference taken earlier."""

    def __init__(self, model, batch, samples_per_frame=256):
        from packages.models.Audio_Net import DeepVAD_audio
        from packages.models.AV_Net import DeepVAD_AV
        from packages.models.Video_Net import DeepVAD_video
        if isinstance(model, DeepVAD_AV):
            if model.use_mcb:
                raise L.AvvadError("DeepVAD_AV(use_mcb=True) cannot be streamed: its fusion divides by the L2 norm of the "
                                   "whole (B, T, 1024) tensor, which is neither causal nor per row")
            self.kind, self.lstm, self.linear = "av", model.lstm_merged, model.vad_merged
        elif isinstance(model, DeepVAD_audio):
            self.kind, self.lstm, self.linear = "audio", model.lstm_audio, model.vad_audio
        elif isinstance(model, DeepVAD_video):
            self.kind, self.lstm, self.linear = "video", model.lstm_video, model.vad_video
        else:
            raise L.AvvadError("a session streams DeepVAD_audio, DeepVAD_video or DeepVAD_AV, not %s" % type(model).__name__)
        if model.training:
            raise L.AvvadError("a session needs the model in eval() mode (training-mode BatchNorm uses batch statistics)")
        if int(batch) < 1:
            raise L.AvvadError("batch must be >= 1")
        if not torch.cuda.is_available():
            raise L.AvvadError("streaming inference needs the GPU: the AV-VAD hot path has no CPU fallback")
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise L.AvvadError("the model must be on the GPU: no CPU fallback")
        self.model, self.batch, self.device = model, int(batch), dev
        self.enc = getattr(model, "wavenet_en", None) if self.kind != "video" else None
        nl, H = self.lstm.num_layers, self.lstm.hidden_size
        self.h = torch.zeros(nl, self.batch, H, dtype=torch.float32, device=dev)
        self.c = torch.zeros_like(self.h)
        self._spare = (torch.zeros_like(self.h), torch.zeros_like(self.h))   # a step writes here, then the pairs swap
        self.enc_state = self.clock = None
        if self.enc is not None:
            self.clock = FrameClock(self.batch, self.enc.receptive_field, samples_per_frame)
            self.enc_state = ops.wavenet_stream_state(self.enc, self.batch, dev)

    def reset(self, rows=None):
        """Start a new utterance on ``rows`` (all when None)."""
        rows = list(range(self.batch)) if rows is None else [int(r) for r in rows]
        if any(r < 0 or r >= self.batch for r in rows):
            raise L.AvvadError("rows must be in [0, %d)" % self.batch)
        idx = torch.tensor(rows, dtype=torch.long, device=self.device)
        self.h.index_fill_(1, idx, 0.0)
        self.c.index_fill_(1, idx, 0.0)
        if self.enc is not None:
            self.enc_state.index_fill_(0, idx, 0.0)
            self.clock.reset(rows)

    def _audio_frames(self, audio, lengths, samples, video=None, with_video=False):
        """-> (audio features (B, T, F), frames per row, video features (B, T, 512) or None).  Every argument is checked
        and the video features -- which touch no state -- are formed before the encoder state and the clock change, so
        a bad argument (a video of the wrong size included) leaves the session as it was.  What is left: a failure
        AFTER the encoder has run (an allocation failure in the LSTM, say) leaves the encoder one chunk ahead of the
        LSTM; ``reset`` the rows then.  With ``with_video`` (AV model) the video must hold the frames the audio yields."""
        B = self.batch
        video_t = self._check_video(video, True) if with_video else None
        if self.enc is None:
            if samples is not None:
                raise L.AvvadError("`samples` only applies to a model with the encoder")
            a = ops._dev(audio, "audio")
            if a.dim() != 3 or a.shape[0] != B or a.shape[1] < 1:
                raise L.AvvadError("audio must be (%d, t >= 1, F) features, got %s" % (B, tuple(a.shape)))
            if video_t is not None and video_t != a.shape[1]:
                raise L.AvvadError("the audio holds %d frames but the video holds %d" % (a.shape[1], video_t))
            frames = _int_list(lengths, B, "lengths", a.shape[1])
            return a, frames, (self._video_feats(video) if with_video else None)
        a = ops._dev(audio, "audio")
        if a.dim() != 3 or a.shape[0] != B or a.shape[1] != self.enc.quantization_channel or a.shape[2] < 1:
            raise L.AvvadError("audio must be (%d, %d, n >= 1) samples, got %s"
                               % (B, self.enc.quantization_channel, tuple(a.shape)))
        n = _int_list(samples, B, "samples", a.shape[2])
        frames = self.clock.plan(n)
        if lengths is not None and _int_list(lengths, B, "lengths", max(frames + [0])) != frames:
            raise L.AvvadError("lengths %s do not match the frames the audio yields, %s" % (list(lengths), frames))
        if video_t is not None and video_t != max(frames):
            raise L.AvvadError("the audio yields %d frames but the video holds %d" % (max(frames), video_t))
        vfeats = self._video_feats(video) if with_video and max(frames) > 0 else None
        feats = ops.wavenet_stream(a, n, self.clock.skip, self.enc, self.enc_state, self.clock.k, max(frames))
        self.clock.advance(n)
        return feats, frames, vfeats

    def step(self, audio=None, video=None, lengths=None, samples=None):
        """The next chunk of every row: the tensors ``model.forward`` takes, for the next few frames only.

        audio: (B, t, 513) features, or (B, qc, n) samples when the model carries the encoder; video: (B, t, 67, 67).
        ``lengths`` (0 <= lengths[b] <= t): how many frames of the chunk are real for row b (default: all); a row with 0
        keeps its state bit for bit.  With the encoder ``samples`` says how many of the n samples are real per row
        (default: all); the frame count follows from it (``FrameClock``), ``lengths`` if given must agree, and for the AV
        model the video must hold exactly that many frames.  -> logits (B, t, y_dim) of exactly these frames; like the
        packed-sequence forward, the LSTM output of a padded position is zero (its logit is the Linear layer's bias)."""
        B = self.batch
        with torch.no_grad():
            if self.kind == "video":
                if audio is not None or samples is not None:
                    raise L.AvvadError("the video model takes no audio")
                self._check_video(video, False)
                x = self._video_feats(video)
                frames = _int_list(lengths, B, "lengths", x.shape[1])
            elif self.kind == "audio":
                if video is not None:
                    raise L.AvvadError("the audio model takes no video")
                x, frames, _ = self._audio_frames(audio, lengths, samples)
            else:
                a, frames, v = self._audio_frames(audio, lengths, samples, video, with_video=True)
                x = a if a.shape[1] == 0 else ops.ConcatColsFn.apply(a, v)
            if x.shape[1] == 0:                      # every row is still warming up
                return torch.zeros(B, 0, self.linear.out_features, dtype=torch.float32, device=self.device)
            old = (self.h, self.c)
            y, (self.h, self.c) = ops.lstm_stack_state(x, frames, self.lstm, state=old, out=self._spare)
            self._spare = old
            return ops.LinearFn.apply(y, self.linear.weight, self.linear.bias)

    def _check_video(self, video, may_be_empty):
        """-> frames the video tensor holds (0 for None where that is allowed)"""
        if video is None and may_be_empty:
            return 0
        if not isinstance(video, torch.Tensor) or not video.is_cuda:
            raise L.AvvadError("video must be a GPU tensor: no CPU fallback")
        if video.dim() != 4 or video.shape[0] != self.batch or (video.shape[1] < 1 and not may_be_empty):
            raise L.AvvadError("video must be (%d, t >= 1, H, W), got %s" % (self.batch, tuple(video.shape)))
        if video.dtype != torch.float32 or video.shape[2] < 32 or video.shape[3] < 32:      # what the trunk accepts
            raise L.AvvadError("video must be float32 frames of at least 32 x 32 (H, W), got %s %s"
                               % (video.dtype, tuple(video.shape)))
        return video.shape[1]

    def _video_feats(self, video):
        return avnn.video_features(self.model.features, ops._dev(video, "video"), False)


def open(model, batch, samples_per_frame=256):
    """A :class:`Session` for ``batch`` streams of ``model`` (``DeepVAD_audio`` / ``DeepVAD_video`` / ``DeepVAD_AV`` with
    concat fusion, in ``eval()`` mode, on the GPU).  ``samples_per_frame`` (the STFT hop by default) is the number of
    encoder output columns averaged into one frame when the model carries the encoder; its ``en_pool_kernel_size`` is a
    whole-utterance output count and has no meaning here."""
    return Session(model, batch, samples_per_frame)


def forward_chunked(model, audio=None, video=None, lengths=None, chunk_frames=1, samples_per_frame=256):
    """``model.eval()(...)`` evaluated through a session in chunks of ``chunk_frames`` frames: same arguments as the
    model's forward (audio features (B,T,F) or, with the encoder, samples (B,qc,RF-1+T*k) whose first chunk carries the
    warm-up), same (B, T, y_dim) result."""
    c = int(chunk_frames)
    if c < 1:
        raise L.AvvadError("chunk_frames must be >= 1")
    ref = audio if audio is not None else video
    B = ref.shape[0]
    sess = open(model, B, samples_per_frame)
    if sess.enc is None:
        T = (audio if sess.kind != "video" else video).shape[1]
    else:
        k, warm = sess.clock.k, sess.clock.warmup
        T = (audio.shape[2] - warm) // k if audio.shape[2] > warm else 0
        if T < 1 or warm + T * k != audio.shape[2]:
            raise L.AvvadError("chunked evaluation of a waveform needs RF-1 + T*%d samples (RF = %d), got %d"
                               % (k, warm + 1, audio.shape[2]))
    lens = _int_list(lengths, B, "lengths", T)
    bias = sess.linear.bias.detach()
    outs = []
    for t0 in range(0, T, c):
        t1 = min(t0 + c, T)
        ln = [min(max(l - t0, 0), t1 - t0) for l in lens]
        tl = max(ln)                                   # frames any row still has in this chunk
        if tl > 0 and sess.enc is None:
            v = video[:, t0:t0 + tl].contiguous() if video is not None else None
            y = sess.step(audio[:, t0:t0 + tl].contiguous() if audio is not None else None, v, ln)
        elif tl > 0:
            # rows are aligned in time; a row is fed its warm-up and whole frames up to its own length, nothing after it
            s0 = 0 if t0 == 0 else warm + t0 * k
            smp = [sess.clock.skip[b] + l * k if l > 0 else 0 for b, l in enumerate(ln)]
            v = video[:, t0:t0 + tl].contiguous() if video is not None else None
            y = sess.step(audio[:, :, s0:warm + (t0 + tl) * k].contiguous(), v, ln, samples=smp)
        else:
            y = bias.new_zeros(B, 0, bias.numel())
        if y.shape[1] < t1 - t0:                       # positions past every row's length: Linear of a zero LSTM output
            y = torch.cat([y, bias.expand(B, t1 - t0 - y.shape[1], bias.numel())], dim=1)
        outs.append(y)
    return torch.cat(outs, dim=1)
