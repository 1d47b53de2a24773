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


class _RowClock:
    """What the clocks of the streaming stages share: the per-row lists named in ``_lists`` and ``ended``, ``reset``, the
    checks every call gets, and -- for a stage that turns ``total`` items taken into ``emitted`` items given, with
    ``pending`` of them held in its state -- the ``plan`` / ``advance`` pair.  Such a clock supplies ``_emitted`` and
    ``_held``; ``advance``'s return value is each clock's own."""
    _lists = ("total", "emitted", "pending")
    _unit = "sample"

    def _rows(self, batch):
        for k in self._lists:
            setattr(self, k, [0] * int(batch))
        self.ended = [False] * int(batch)

    def reset(self, rows=None):
        for b in (range(len(self.ended)) if rows is None else rows):
            for k in self._lists:
                getattr(self, k)[b] = 0
            self.ended[b] = False

    def _final(self, final, B):
        return set(ops._ints(final))

    def _checked(self, n, final):
        """-> (counts per row, the rows that end): one count >= 0 per row, ``final`` within the rows, and a row that ended
        neither fed nor ended again before its reset."""
        B = len(self.ended)
        n = ops._ints(n)
        if len(n) != B or (n and min(n) < 0):
            raise L.AvvadError("one %s count >= 0 per row expected (%d), got %s" % (self._unit, B, n))
        final = self._final(final, B)
        if final and (min(final) < 0 or max(final) >= B):
            raise L.AvvadError("final rows must be in [0, %d)" % B)
        for b in (range(B) if True in self.ended else ()):
            if self.ended[b] and (n[b] > 0 or b in final):
                raise L.AvvadError("row %d ended with a final call: reset it before it takes %ss again" % (b, self._unit))
        return n, final

    def _plan(self, n, final):
        """-> per row (total, emitted, pending, ended) after the call; a row that ended idles until its reset"""
        n, final = self._checked(n, final)
        after = []
        for b, nb in enumerate(n):
            if self.ended[b]:
                after.append((self.total[b], self.emitted[b], self.pending[b], True))
            else:
                N, last = self.total[b] + nb, b in final
                e = self._emitted(b, N, last)
                after.append((N, e, self._held(N, e), last))
        return after

    def plan(self, n, final=()):
        """Items each row emits from ``n[b]`` more (rows in ``final`` end with them); raises :class:`AvvadError` when a
        count is negative or a row that ended is fed again.  Changes nothing."""
        return [row[1] - e for row, e in zip(self._plan(n, final), self.emitted)]

    def _advance(self, n, final):
        """``plan`` and then commit: -> (total, emitted, pending, ended as they applied to THIS call, items each row emits)"""
        after = self._plan(n, final)
        before = (list(self.total), list(self.emitted), list(self.pending), list(self.ended))
        for b, row in enumerate(after):
            self.total[b], self.emitted[b], self.pending[b], self.ended[b] = row
        return before + ([e - e0 for e, e0 in zip(self.emitted, before[1])],)


class SampleClock(_RowClock):
    """Host-side bookkeeping of the streaming STFT front-end, per row, beside :class:`FrameClock`: ``total`` samples
    taken since the reset, ``emitted`` frames, and ``pending`` = total - emitted * hop < n_fft samples held in the
    front-end state (they completed no frame yet, or later frames still overlap them).  After N samples a row has
    emitted max(0, (N - n_fft) // hop + 1) frames, so a frame may straddle any number of calls.  A row named in ``final``
    ends with that call and also yields what ``ops.n_frames(N)`` -- the reference's count, one-hop end pad and its float
    test included -- has beyond that (0 or 1 frame, read with zeros behind the last sample); it must be ``reset`` before
    it takes samples again."""

    def __init__(self, batch, n_fft=1024, hop=256):
        if int(batch) < 1 or int(n_fft) < 1 or int(hop) < 1 or int(hop) > int(n_fft):
            raise L.AvvadError("SampleClock needs batch >= 1 and 1 <= hop <= n_fft")
        self.n_fft, self.hop = int(n_fft), int(hop)
        self._rows(batch)

    def _going(self, N):
        """frames a row that goes on has emitted after N samples"""
        return max(0, (N - self.n_fft) // self.hop + 1)

    def _emitted(self, b, N, last):
        if not last:
            return max(0, (N - self.n_fft) // self.hop + 1)
        e = max(ops.n_frames(N, self.n_fft, self.hop), 0)
        if not 0 <= e - self._going(N) <= 1:        # cannot happen for the reference's framing; never emit a wrong count
            raise L.AvvadError("row %d: %d samples end %d frames away from the reference's count" % (b, N, e - self._going(N)))
        return e

    def _held(self, N, e):
        return max(N - e * self.hop, 0)

    def advance(self, n, final=()):
        """``plan`` and then consume: -> (frames per row, the pending counts that applied to THIS call, per row 1 where
        the last frame is the zero-padded one)."""
        _, _, used, was_ended, frames = self._advance(n, final)
        pad = [0] * len(frames)
        for b in (range(len(pad)) if self.ended != was_ended else ()):      # the rows that ended with this call
            if not was_ended[b]:
                pad[b] = self.emitted[b] - self._going(self.total[b])
        return frames, used, pad


class RateClock(_RowClock):
    """Host-side bookkeeping of the streaming resampler (``ops.resample_stream``), per row, beside :class:`SampleClock`:
    ``total`` input samples taken since the reset, ``emitted`` output samples, and ``pending`` -- the inputs the next output
    still needs of those that came, at most ``H - 2`` of the ``H = 2 * half // up + 2`` the state holds.  With
    ``half = 10 * max(up, down)``, a row that goes on has emitted ``floor((N * up - 1 - half) / down) + 1`` samples after N
    inputs (0 while ``N * up - 1 - half < 0``): the outputs whose every tap has arrived.  A row named in ``final`` ends with
    that call and emits up to ``ceil(N * up / down)``, so a stream of N samples yields the whole-utterance call's count; it
    must be ``reset`` before it takes samples again.  ``total`` (with ``emitted`` to match, see ``preset``) may be set ahead
    for a test of large positions."""

    def __init__(self, batch, up, down):
        self.up, self.down = ops._ratio_check(up, down)
        if int(batch) < 1:
            raise L.AvvadError("RateClock needs batch >= 1")
        self.half = 10 * max(self.up, self.down)
        self._rows(batch)

    def count(self, N):
        """outputs a row that goes on has emitted after N inputs"""
        a = int(N) * self.up - 1 - self.half
        return a // self.down + 1 if a >= 0 else 0

    def _held(self, N, e):
        """inputs of the first N that output e (the next one) still needs"""
        first = max(0, -((self.half - e * self.down) // self.up))      # ceil((e down - half) / up)
        return max(N - first, 0)

    def preset(self, row, total):
        """Puts ``row`` where a stream stands after ``total`` inputs (a test of positions beyond 2^31 costs nothing)."""
        self.total[row] = int(total)
        self.emitted[row] = self.count(total)
        self.pending[row] = self._held(self.total[row], self.emitted[row])
        self.ended[row] = False

    def _emitted(self, b, N, last):
        return max((N * self.up + self.down - 1) // self.down if last else self.count(N), self.emitted[b])

    def advance(self, n, final=()):
        """``plan`` and then consume: -> (inputs each row had behind it, outputs it had emitted, outputs of THIS call)."""
        total, emitted, _, _, n_emit = self._advance(n, final)
        return total, emitted, n_emit


class OlaClock(_RowClock):
    """Host-side bookkeeping of the streaming overlap-add (``ops.istft_stream``), per row, beside :class:`SampleClock`:
    ``emitted`` frames taken and ``written`` samples returned since the reset.  A row that goes on writes
    ``frames[b] * hop`` samples per call -- those no later frame can cover -- so ``written = emitted * hop``.  A row that
    ends with N input samples (``final_totals``) writes the ``N - written[b]`` that are left: a stream of N samples
    yields exactly N, as ``ops.resynth`` returns exactly L_b, and a row that never completes a frame yields N zeros at
    its end.  It must be ``reset`` before it takes frames again."""
    _lists = ("emitted", "written")
    _unit = "frame"

    def __init__(self, batch, n_fft=1024, hop=256):
        if int(batch) < 1 or int(n_fft) < 1 or int(hop) < 1 or int(hop) > int(n_fft):
            raise L.AvvadError("OlaClock needs batch >= 1 and 1 <= hop <= n_fft")
        self.n_fft, self.hop = int(n_fft), int(hop)
        self._rows(batch)

    def _final(self, final_totals, B):
        if final_totals is None:
            return {}
        if not isinstance(final_totals, dict):
            if len(final_totals) != B:
                raise L.AvvadError("final_totals must be {row: samples} or hold one entry (None: the row goes on) per row")
            final_totals = {b: n for b, n in enumerate(final_totals) if n is not None}
        return {int(b): int(n) for b, n in final_totals.items()}

    def _plan(self, frames, final_totals):
        frames, fin = self._checked(frames, final_totals)
        for b, n in fin.items():
            if n < self.written[b]:
                raise L.AvvadError("row %d: a stream of %d samples cannot end after %d were written" % (b, n, self.written[b]))
        return frames, [fin[b] - self.written[b] if b in fin else f * self.hop for b, f in enumerate(frames)], fin

    def plan(self, frames, final_totals=None):
        """-> (frames each row has behind it, samples each row writes) for a call with ``frames[b]`` more frames, rows in
        ``final_totals`` ({row: N input samples}, or a list with None for rows that go on) ending with it; raises
        :class:`AvvadError` when a count is negative or a row that ended is fed again.  Changes nothing."""
        return list(self.emitted), self._plan(frames, final_totals)[1]

    def advance(self, frames, final_totals=None):
        """``plan`` and then consume: -> (n_before, n_out)."""
        frames, n_out, fin = self._plan(frames, final_totals)
        before = list(self.emitted)
        for b, f in enumerate(frames):
            self.emitted[b] += f
            self.written[b] += n_out[b]
            self.ended[b] = self.ended[b] or b in fin
        return before, n_out


def _int_list(v, B, what, hi):
    """``ops._ints``: one value in [0, hi] per row, None standing for hi"""
    return ops._ints(v, B, hi, default=hi, what=what)


class _Stage:
    """One streaming stage of a session's waveform front-end: its host ``clock`` (None: the stage is not in the path) and,
    once ``build`` ran, its table on the GPU (basis or taps), its ``state`` and the ``spare`` a call writes the new state
    to before the two swap."""

    def __init__(self, clock=None):
        self.clock = clock
        self.table = self.state = self.spare = None

    @property
    def built(self):
        return self.state is not None

    def build(self, table, state):
        self.table, self.state, self.spare = table, state, torch.zeros_like(state)

    def reset(self, rows, idx):
        if self.clock is not None:
            self.clock.reset(rows)
        if self.state is not None:
            self.state.index_fill_(0, idx, 0.0)

    def swap(self):
        self.state, self.spare = self.spare, self.state


def _stage_attr(stage, field):
    """a session attribute that lives in one of its stages: readable and assignable, as callers save and restore them"""
    return property(lambda s: getattr(getattr(s, stage), field), lambda s, v: setattr(getattr(s, stage), field, v))


class Session:
    """State of ``batch`` streams of one model.  Attributes a caller may save, restore or move between sessions:
    ``h`` / ``c`` (num_layers, batch, H) LSTM state, ``enc_state`` (batch, floats) encoder state (None without an
    encoder; all zeros = start of utterance) and ``clock.skip`` (host list: remaining warm-up samples per row).  A step
    writes the new LSTM state into a spare pair of tensors and swaps, so read ``h`` / ``c`` from the session after each
    step, not from a reference taken earlier."""
    # the waveform front-end of the spectrogram models: the STFT (step_wave), the overlap-add behind it (step_enhance) and
    # the resampler in front of it (set_frontend(fs_in=...); no clock at 16 kHz).  The clocks are host bookkeeping and
    # exist from the start; the GPU side is built by prepare_frontend on first use.
    sample_clock, stft_state = _stage_attr("_stft", "clock"), _stage_attr("_stft", "state")
    ola_clock, ola_state = _stage_attr("_ola", "clock"), _stage_attr("_ola", "state")
    rate_clock, rs_state = _stage_attr("_rs", "clock"), _stage_attr("_rs", "state")

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
        self._route = [None] * self.batch          # per row: "wave" / "enhance" once it has taken samples since its reset
        self._frontend = dict(stats=None, eps=1e-8, n_fft=1024, hop=256, fs_in=16000)
        self._stages(1024, 256, 1, 1, self.kind != "video" and self.enc is None)
        self.peak = torch.ones(self.batch, dtype=torch.float32, device=dev)
        if self.enc is not None:
            self.clock = FrameClock(self.batch, self.enc.receptive_field, samples_per_frame)
            self.enc_state = ops.wavenet_stream_state(self.enc, self.batch, dev)

    def _stages(self, n_fft, hop, up, down, wave=True):
        """fresh front-end stages (``wave`` False: a model that takes no waveform this way has none of the clocks)"""
        self._stft = _Stage(SampleClock(self.batch, n_fft, hop) if wave else None)
        self._ola = _Stage(OlaClock(self.batch, n_fft, hop) if wave else None)
        self._rs = _Stage(RateClock(self.batch, up, down) if wave and up != down else None)

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
        self.peak.index_fill_(0, idx, 1.0)
        for stage in (self._stft, self._ola, self._rs):
            stage.reset(rows, idx)
        for r in rows:
            self._route[r] = None

    # ------------------------------------------------------------------ waveform front-end (csrc/stft_stream.hip)
    def _wave_check(self):
        if self.kind == "video" or self.enc is not None:
            raise L.AvvadError("step_wave feeds the STFT front-end of DeepVAD_audio / DeepVAD_AV without the encoder; "
                               "a model with the encoder takes samples through step(), the video model takes none")

    def set_frontend(self, stats=None, eps=1e-8, n_fft=1024, hop=256, fs_in=16000):
        """Configuration of ``step_wave``'s front-end: ``stats`` (``train.Stats``-like: ``get("audio_mean" /
        "audio_std", device)`` and ``.eps``) standardises the log-power features, ``eps`` is the log's.  ``fs_in``: the rate
        of the samples ``step_wave`` / ``step_enhance`` take; another rate than 16000 goes through the streaming resampler
        (``ops.resample_stream``) into the same 16 kHz front-end, and the logits are those of ``ops.resample`` of the whole
        utterance fed at 16 kHz, bit for bit.  Changing ``n_fft`` / ``hop`` / ``fs_in`` starts every row's front-end over."""
        self._wave_check()
        n_fft, hop = ops._n_fft_check(n_fft), int(hop)
        if hop < 1 or hop > n_fft:
            raise L.AvvadError("hop must be in [1, n_fft]")
        up, down = ops.resample_ratio(fs_in, 16000)
        fs_in = int(fs_in)
        if (n_fft, hop) != (self.sample_clock.n_fft, self.sample_clock.hop) or fs_in != self._frontend["fs_in"]:
            self._stages(n_fft, hop, up, down)
            self._route = [None] * self.batch
        self._frontend = dict(stats=stats, eps=float(eps), n_fft=n_fft, hop=hop, fs_in=fs_in)

    def prepare_frontend(self):
        """Builds what ``step_wave`` needs on the GPU -- the windowed basis, ``stft_state`` and its spare -- if it is not
        there yet (``step_wave`` does it on first use; a caller that restores a saved ``stft_state`` does it first).  For a
        model that predicts a mask over the bins (``step_enhance``) also the inverse basis, ``ola_state`` and its spare."""
        self._wave_check()
        B, n_fft, dev, rc = self.batch, self._frontend["n_fft"], self.device, self._rs.clock
        if not self._stft.built:
            self._stft.build(ops.stft_stream_basis(n_fft, dev), ops.stft_stream_state(B, n_fft, dev))
        if rc is not None and not self._rs.built:
            self._rs.build(ops.resample_taps_on(rc.up, rc.down, dev), ops.resample_stream_state(B, rc.up, rc.down, dev))
        if not self._ola.built and self.linear.out_features == n_fft // 2 + 1:
            self._ola.build(ops.istft_stream_basis(n_fft, dev), ops.istft_stream_state(B, n_fft, dev))

    def plan_wave(self, samples, final=()):
        """Frames each row yields from ``samples[b]`` more samples at ``fs_in`` (rows in ``final`` end with them): the
        resampler's clock composed with the STFT's, which is what tells an AV caller how many lip frames a packet needs.
        Changes nothing."""
        self._wave_check()
        n = ops._ints(samples)
        if self.rate_clock is not None:
            n = self.rate_clock.plan(n, final)
        return self.sample_clock.plan(n, final)

    def step_wave(self, wave, samples=None, video=None, final=None):
        """The next SAMPLES of every row of a spectrogram model: wave (B, n) float32 on the GPU, of which row b's first
        ``samples[b]`` are real (default: all n; any count >= 0 -- a frame may straddle calls).  Each sample is divided by
        ``self.peak[b]``; the frames the samples complete go through the STFT front-end (``set_frontend``) and the model.
        ``final``: rows whose utterance ends with this call (they also yield the reference's zero-padded last frame;
        ``reset`` them before they take samples again).  For the AV model ``video`` must hold exactly
        ``max(self.plan_wave(samples, final))`` lip frames (None when that is 0).  With ``set_frontend(fs_in=...)`` the
        samples are at that rate.
        -> (logits (B, tmax, y_dim), frames per row); (B, 0, y_dim) when no row completes a frame."""
        return self._step_samples(wave, samples, video, final, None)

    def step_enhance(self, wave, samples=None, video=None, final=None, hard=True):
        """``step_wave`` for a model that predicts a mask over the bins (``y_dim == n_fft // 2 + 1``), which also returns
        the ENHANCED samples: the logits of the frames the samples complete mask those frames' spectrum (``hard``: logit > 0,
        the evaluators' sigmoid > 0.5; else ``sigmoid(logit)``), and the streaming inverse STFT (``ops.istft_stream``) turns
        it back into samples, multiplied by ``self.peak[b]``.  A sample comes out once no later frame can cover it, up to
        ``n_fft - 1`` samples after it went in; a row in ``final`` returns all that is left, so a stream of N samples
        returns exactly N (at ``fs_in`` other than 16000: the enhanced samples are 16 kHz, ``ops.resample_length(N)`` of
        them).  The cost of a call does not depend on the position in the utterance, and any split of a stream
        into packets gives the same samples bit for bit (given the same logits).  A row goes through ONE of ``step_wave`` /
        ``step_enhance`` from its reset to its end.
        -> (logits (B, tmax, y_dim), frames per row, enhanced (B, nmax) with zeros behind a row's count, samples per row)."""
        return self._step_samples(wave, samples, video, final, bool(hard))

    def _step_samples(self, wave, samples, video, final, hard):
        """the body of ``step_wave`` (``hard`` None) and ``step_enhance``"""
        self._wave_check()
        B = self.batch
        enhance = hard is not None
        if enhance and self.linear.out_features != self._frontend["n_fft"] // 2 + 1:
            raise L.AvvadError("step_enhance needs a model that predicts a mask over the %d bins, this one has y_dim = %d"
                               % (self._frontend["n_fft"] // 2 + 1, self.linear.out_features))
        if not isinstance(wave, torch.Tensor) or not wave.is_cuda:
            raise L.AvvadError("wave must be a GPU tensor: no CPU fallback")
        if wave.dtype != torch.float32 or wave.dim() != 2 or wave.shape[0] != B:
            raise L.AvvadError("wave must be (%d, n) float32 samples, got %s %s" % (B, wave.dtype, tuple(wave.shape)))
        n = _int_list(samples, B, "samples", wave.shape[1])
        self.prepare_frontend()
        rs, stft, ola = self._rs, self._stft, self._ola
        final = () if final is None else final
        n_in = n
        if rs.clock is not None:                    # the samples are at fs_in: the 16 kHz counts they resample to
            n = rs.clock.plan(n_in, final)
        frames = stft.clock.plan(n, final)
        tmax = max(frames)
        route = "enhance" if enhance else "wave"
        fin = set(ops._ints(final))
        live = [b for b in range(B) if n_in[b] > 0 or b in fin]
        for b in live:
            if self._route[b] not in (None, route):
                raise L.AvvadError("row %d went through step_%s since its reset: a row stays with one of step_wave / "
                                   "step_enhance until its end" % (b, self._route[b]))
        totals = {b: stft.clock.total[b] + n[b] for b in fin}
        if enhance:
            ola.clock.plan(frames, totals)
        with torch.no_grad():
            vfeats = None
            if self.kind == "av":
                vt = self._check_video(video, True)
                if vt != tmax:
                    raise L.AvvadError("the samples yield %d frames but the video holds %d" % (tmax, vt))
                vfeats = self._video_feats(video) if tmax > 0 else None
            elif video is not None:
                raise L.AvvadError("the audio model takes no video")
            f = self._frontend
            mean = std = None
            if f["stats"] is not None:
                mean, std = f["stats"].get("audio_mean", self.device), f["stats"].get("audio_std", self.device)
            if rs.clock is not None:
                wave, n = ops.resample_stream(wave, n_in, rs.clock, rs.state, rs.table, final, rs.spare)
                rs.swap()
            res = ops.stft_stream(wave, n, stft.clock, stft.state, stft.table, self.peak, mean, std, final, stft.spare,
                                  eps=f["eps"], norm_eps=f["stats"].eps if f["stats"] is not None else f["eps"],
                                  return_spec=enhance)
            x, frames = res[0], res[1]
            stft.swap()
            for b in live:
                self._route[b] = route
            if tmax == 0:
                logits = torch.zeros(B, 0, self.linear.out_features, dtype=torch.float32, device=self.device)
            else:
                if vfeats is not None:
                    x = ops.ConcatColsFn.apply(x, vfeats)
                old = (self.h, self.c)
                y, (self.h, self.c) = ops.lstm_stack_state(x, frames, self.lstm, state=old, out=self._spare)
                self._spare = old
                logits = ops.LinearFn.apply(y, self.linear.weight, self.linear.bias)
            if not enhance:
                return logits, frames
            if tmax == 0 and not fin:                   # no row has a frame or ends: nothing comes out, no state moves
                return logits, frames, torch.zeros(B, 0, dtype=torch.float32, device=self.device), [0] * B
            enhanced, n_out = ops.istft_stream(res[2], frames, ola.clock, ola.state, ola.table, logits if tmax else None,
                                               3 if hard else 2, self.peak, totals, ola.spare)
            ola.swap()
            return logits, frames, enhanced, n_out

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


def _open_wave_chunked(model, wave, lengths, chunk_samples, stats, peak, eps, n_fft, hop, fs_in=16000):
    """the shared opening of ``forward_wave_chunked`` / ``enhance_wave_chunked``: the arguments checked, a session with its
    front-end built and ``peak`` set.  -> (chunk_samples, wave (B, Lmax), lengths (list), session)"""
    c = int(chunk_samples)
    if c < 1:
        raise L.AvvadError("chunk_samples must be >= 1")
    w = ops._wave2d(wave)[1]
    if w.dim() != 2:
        raise L.AvvadError("wave must be (B, L) samples, got %s" % (tuple(w.shape),))
    B, Lmax = w.shape
    lens = _int_list(lengths, B, "lengths", Lmax)
    sess = open(model, B)
    sess.set_frontend(stats, eps, n_fft, hop, fs_in)
    sess.prepare_frontend()
    if peak is not None:
        sess.peak.copy_(ops._row_vector(peak, B, "peak"))
    return c, w, lens, sess


def _packets(lens, c, ends):
    """The packets of ``c`` samples that feed rows of ``lens`` samples: yields (s0, samples per row, the rows of ``ends``
    whose last sample the packet holds -- each once, in the first packet that reaches its end)."""
    ended = set()
    for s0 in range(0, max(max(lens), 1), c):
        fin = [b for b in range(len(lens)) if ends[b] and b not in ended and s0 + c >= lens[b]]
        ended.update(fin)
        yield s0, [min(max(l - s0, 0), c) for l in lens], fin


def _scatter(out, done, y, counts):
    """row b's first ``counts[b]`` items of ``y`` go behind the ``done[b]`` it has in ``out``"""
    for b, k in enumerate(counts):
        if k > 0:
            out[b, done[b]:done[b] + k] = y[b, :k]
            done[b] += k


def forward_wave_chunked(model, wave, lengths=None, video=None, chunk_samples=256, stats=None, peak=None, eps=1e-8,
                         n_fft=1024, hop=256, max_frames=None, fs_in=16000):
    """A spectrogram model (``DeepVAD_audio`` / concat ``DeepVAD_AV`` without the encoder, in ``eval()`` mode) scored
    from RAW SAMPLES through a session: wave (B, Lmax) on the GPU, row b's first ``lengths[b]`` samples real, fed in
    packets of ``chunk_samples`` with each row's last packet ``final``.  ``peak`` (B,) is what every sample is divided by
    (``ops.peak(wave)`` reproduces the evaluators' x / max|x|; None: 1), ``stats`` standardises the features, ``video``
    (B, T, 67, 67) holds the lip frames already decoded and standardised.  ``max_frames[b]`` ends row b after that many
    frames (the evaluators' crop to the label length).  -> logits (B, T, y_dim), T = the longest row's frame count
    (``ops.n_frames``, capped by ``max_frames``); positions behind a row's frames hold the Linear layer's bias.
    ``fs_in``: the rate of ``wave`` and of the packets (``Session.set_frontend``); the frames are those of the utterance
    resampled to 16 kHz, and ``peak`` is what the samples are divided by behind the resampler."""
    c, w, lens, sess = _open_wave_chunked(model, wave, lengths, chunk_samples, stats, peak, eps, n_fft, hop, fs_in)
    B, Lmax = w.shape
    rc = sess.rate_clock
    total = [max(ops.n_frames(l if rc is None else ops.resample_length(l, rc.up, rc.down), n_fft, hop), 0) for l in lens]
    ends = [True] * B                                   # the row ends with its last sample (and may owe the padded frame)
    if max_frames is not None:
        for b, mf in enumerate(_int_list(max_frames, B, "max_frames", 1 << 30)):
            if mf < total[b] and rc is None:            # exactly mf frames: the samples they need and no end
                total[b], ends[b] = mf, False
                lens[b] = (mf - 1) * hop + n_fft if mf > 0 else 0
            elif mf < total[b]:                         # at another rate the row runs to its end and the frames past mf are dropped
                total[b] = mf
    T = max(total)
    if sess.kind == "av" and (video is None or video.dim() != 4 or video.shape[0] != B or video.shape[1] < T):
        raise L.AvvadError("the AV model needs video (B, >= %d, H, W)" % T)
    bias = sess.linear.bias.detach()
    out = bias.expand(B, T, bias.numel()).clone()
    done = [0] * B
    for s0, n, fin in _packets(lens, c, ends):
        frames = sess.plan_wave(n, fin)
        tl = max(frames)
        v = None
        if sess.kind == "av" and tl > 0:                # every row's next lip frames start where its own frames stand
            v = video.new_zeros((B, tl) + tuple(video.shape[2:]))
            for b, f in enumerate(frames):
                f = min(f, video.shape[1] - done[b])
                if f > 0:
                    v[b, :f] = video[b, done[b]:done[b] + f]
        y, frames = sess.step_wave(w[:, s0:s0 + c].contiguous(), n, v, fin)
        _scatter(out, done, y, [min(f, total[b] - done[b]) for b, f in enumerate(frames)])
    return out


def enhance_wave_chunked(model, wave, lengths=None, chunk_samples=256, stats=None, peak=None, hard=True, eps=1e-8, n_fft=1024,
                         hop=256, fs_in=16000):
    """The twin of ``forward_wave_chunked`` for a mask-predicting ``DeepVAD_audio(y_dim=n_fft // 2 + 1)``: wave (B, Lmax) on
    the GPU, row b's first ``lengths[b]`` samples real, fed through ``Session.step_enhance`` in packets of ``chunk_samples``
    with each row's last packet ``final``.  ``peak`` (B,): what every sample is divided by on the way in and multiplied by
    on the way out (None: 1).  -> enhanced samples (B, Lmax), row b's first ``lengths[b]`` real, zeros behind them.
    ``fs_in``: the rate of ``wave``; the enhanced samples are 16 kHz, (B, ``resample_length(Lmax)``) with
    ``resample_length(lengths[b])`` real ones per row."""
    c, w, lens, sess = _open_wave_chunked(model, wave, lengths, chunk_samples, stats, peak, eps, n_fft, hop, fs_in)
    B, Lmax = w.shape
    rc = sess.rate_clock
    out = w.new_zeros(B, Lmax if rc is None else ops.resample_length(Lmax, rc.up, rc.down))
    done = [0] * B
    for s0, n, fin in _packets(lens, c, [True] * B):
        _, _, y, n_out = sess.step_enhance(w[:, s0:s0 + c].contiguous(), n, None, fin, hard)
        _scatter(out, done, y, n_out)
    return out
