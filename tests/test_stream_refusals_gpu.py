"""The three streaming stages (``ops.stft_stream``, ``ops.istft_stream``, ``ops.resample_stream``) share one contract:
every argument is checked before the clock or a state changes.  A refused call leaves the clock's lists and the state
tensor as they were, and the stream goes on as if the call had never been made.  Smallest shapes: B = 2, n_fft = 64,
hop = 16, 40-sample chunks or 2-frame spectra, the ratio 2/3."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N_FFT, HOP, UP, DOWN = 2, 64, 16, 2, 3
# four calls: row 1 ends with the first and idles, row 0 ends with the last (7 frames of 160 samples for the inverse)
SAMPLES = ([40, 33], [40, 0], [17, 0], [40, 0])
FRAMES = ([2, 1], [2, 0], [1, 0], [2, 0])
ENDS = ([1], [], [], [0])


def _bits(t):
    return t.view(torch.int32)


class _Stage:
    """one stage with its clock, state, spare and table, and the inputs of the four calls"""

    def __init__(self, kind):
        from avvad import ops
        from avvad import stream as S
        g = torch.Generator().manual_seed(11)
        self.kind = kind
        if kind == "istft":
            self.clock, self.fn = S.OlaClock(B, N_FFT, HOP), ops.istft_stream
            self.table, self.other_table = ops.istft_stream_basis(N_FFT, DEV), ops.istft_stream_basis(96, DEV)
            self.state = ops.istft_stream_state(B, N_FFT, DEV)
            self.x = [torch.randn(B, 2, N_FFT // 2 + 1, 2, generator=g).to(DEV) for _ in FRAMES]
            self.counts, self.hi = FRAMES, 2
            self.ends = [{b: {0: 160, 1: 50}[b] for b in e} for e in ENDS]
        else:
            if kind == "stft":
                self.clock, self.fn = S.SampleClock(B, N_FFT, HOP), ops.stft_stream
                self.table, self.other_table = ops.stft_stream_basis(N_FFT, DEV), ops.stft_stream_basis(96, DEV)
                self.state = ops.stft_stream_state(B, N_FFT, DEV)
            else:
                self.clock, self.fn = S.RateClock(B, UP, DOWN), ops.resample_stream
                self.table, self.other_table = ops.resample_taps_on(UP, DOWN, DEV), ops.resample_taps_on(1, 4, DEV)
                self.state = ops.resample_stream_state(B, UP, DOWN, DEV)
            self.x = [torch.randn(B, 40, generator=g).to(DEV) for _ in SAMPLES]
            self.counts, self.hi = SAMPLES, 40
            self.ends = [list(e) for e in ENDS]
        self.spare = torch.full_like(self.state, float("nan"))

    def call(self, i, counts=None, state=None, out_state="spare", table=None):
        """call ``i`` of the stream, with the arguments named replaced; -> (the output, the counts that came with it)"""
        counts = self.counts[i] if counts is None else counts
        state = self.state if state is None else state
        out_state = self.spare if isinstance(out_state, str) else out_state
        table = self.table if table is None else table
        if self.kind == "istft":
            return self.fn(self.x[i], counts, self.clock, state, table, final_samples=self.ends[i], out_state=out_state)
        return self.fn(self.x[i], counts, self.clock, state, table, final=self.ends[i], out_state=out_state)[:2]

    def good(self, i, in_place=False):
        out = self.call(i, out_state=None if in_place else "spare")
        if not in_place:
            self.state, self.spare = self.spare, self.state
        return out

    def lists(self):
        return {k: list(getattr(self.clock, k)) for k in ("total", "emitted", "pending", "written", "ended")
                if hasattr(self.clock, k)}


def _stream(kind, in_place=False, refused=None):
    """the four calls; ``refused(stage)`` runs after the first.  -> (outputs and counts per call, last state, clock lists)"""
    s = _Stage(kind)
    outs = [s.good(0, in_place)]
    if refused is not None:
        refused(s)
    outs += [s.good(i, in_place) for i in (1, 2, 3)]
    return outs, s.state, s.lists()


def _refused(s):
    from avvad import AvvadError
    assert s.clock.ended == [False, True]
    width = s.state.shape[1]
    bad = dict(
        state_shape=dict(state=torch.zeros(B, width + 1, device=DEV)),
        state_dtype=dict(state=s.state.double()),
        out_state_strided=dict(out_state=torch.zeros(width, B, device=DEV).t()),
        table_size=dict(table=s.other_table),
        counts_too_long=dict(counts=[1, 0, 0]),
        count_out_of_range=dict(counts=[s.hi + 1, 0]),
        ended_row_fed=dict(counts=[1, 1]))
    assert bad["out_state_strided"]["out_state"].shape == s.state.shape
    lists, state, spare = s.lists(), s.state.clone(), s.spare.clone()
    for name, args in bad.items():
        with pytest.raises(AvvadError):
            s.call(1, **args)
        assert s.lists() == lists, name
        assert torch.equal(_bits(s.state), _bits(state)) and torch.equal(_bits(s.spare), _bits(spare)), name


@pytest.mark.parametrize("kind", ["stft", "istft", "resample"])
def test_a_refused_stream_call_changes_nothing(kind):
    got, state, lists = _stream(kind, refused=_refused)
    fresh, fresh_state, fresh_lists = _stream(kind)
    in_place, in_place_state, in_place_lists = _stream(kind, in_place=True)       # out_state=None against out_state=spare
    assert lists == fresh_lists == in_place_lists and lists["ended"] == [True, True]
    assert sum(max(n) for _, n in fresh) > 0
    for other, other_state in ((got, state), (in_place, in_place_state)):
        for (a, na), (b, nb) in zip(other, fresh):
            assert na == nb and a.shape == b.shape and torch.equal(_bits(a), _bits(b))
        assert torch.equal(_bits(other_state), _bits(fresh_state))
