"""The rules the three row clocks of the streaming stages share (``SampleClock``, ``RateClock``, ``OlaClock``), at B = 3:
what a call must hold, what a row that ended may still do, what ``reset`` restores, and that ``plan`` and a refused
``advance`` change nothing.  Host bookkeeping only: no GPU, no library."""
import pytest

B = 3
LISTS = ("total", "emitted", "pending", "written", "ended")


def _make(kind):
    """-> (clock, final(rows): the clock's way to say that these rows end, holding 5000 samples each)"""
    from avvad import stream as S
    if kind == "sample":
        return S.SampleClock(B, 64, 16), lambda rows: list(rows)
    if kind == "rate":
        return S.RateClock(B, 2, 3), lambda rows: list(rows)
    return S.OlaClock(B, 64, 16), lambda rows: {b: 5000 for b in rows}


def _lists(c):
    return {k: list(getattr(c, k)) for k in LISTS if hasattr(c, k)}


def _advanced(kind):
    """a clock every row of which has taken something, row 1 ended"""
    c, final = _make(kind)
    c.advance([70, 5, 33])
    c.advance([3, 2, 40], final([1]))
    assert c.ended == [False, True, False]
    return c, final


@pytest.mark.parametrize("kind", ("sample", "rate", "ola"))
def test_what_a_call_must_hold(kind):
    from avvad import AvvadError
    c, final = _advanced(kind)
    before = _lists(c)
    for counts, fin in (([1, 0], final([])), ([1, 0, 1, 1], final([])), ([], final([])),      # not one count per row
                        ([1, 0, -1], final([])), ([-2, 0, 0], final([0])),                   # a negative count
                        ([1, 0, 1], final([B])), ([1, 0, 1], final([-1])), ([0, 0, 0], final([0, 7]))):     # final out of range
        with pytest.raises(AvvadError):
            c.plan(counts, fin)
        with pytest.raises(AvvadError):
            c.advance(counts, fin)
        assert _lists(c) == before, (counts, fin)


@pytest.mark.parametrize("kind", ("sample", "rate", "ola"))
def test_a_row_that_ended_idles_until_its_reset(kind):
    from avvad import AvvadError
    c, final = _advanced(kind)
    before = _lists(c)
    for counts, fin in (([0, 1, 0], final([])), ([0, 0, 0], final([1])), ([4, 9, 4], final([1]))):
        with pytest.raises(AvvadError, match="reset"):
            c.plan(counts, fin)
        with pytest.raises(AvvadError, match="reset"):
            c.advance(counts, fin)
        assert _lists(c) == before, (counts, fin)
    planned = c.plan([0, 0, 0], final([]))                            # it may idle with 0 ...
    out = c.advance([0, 0, 0], final([]))
    assert _lists(c) == before
    assert (planned[1] if kind == "ola" else planned) == [0, 0, 0] and out[-1 if kind != "sample" else 0] == [0, 0, 0]
    c.advance([16, 0, 16], final([]))                                 # ... while the others go on
    assert _lists(c)["ended"] == [False, True, False] and all(_lists(c)[k][1] == before[k][1] for k in before)


@pytest.mark.parametrize("kind", ("sample", "rate", "ola"))
def test_reset_restores_exactly_the_rows_named(kind):
    c, final = _advanced(kind)
    fresh = _lists(_make(kind)[0])
    before = _lists(c)
    assert all(any(before[k][b] != fresh[k][b] for k in before) for b in range(B)), "every row must have moved"
    c.reset([1])
    after = _lists(c)
    for k in after:
        assert after[k][1] == fresh[k][1] and after[k][0] == before[k][0] and after[k][2] == before[k][2], k
    c.advance([5, 5, 5], final([]))                                   # the row takes items again
    c.reset()
    assert _lists(c) == fresh


@pytest.mark.parametrize("kind", ("sample", "rate", "ola"))
def test_plan_changes_nothing_and_tells_what_advance_returns(kind):
    c, final = _make(kind)
    calls = [([70, 5, 33], []), ([0, 64, 1], []), ([3, 2, 40], [1]), ([16, 0, 0], []), ([1, 0, 17], [0, 2]), ([0, 0, 0], [])]
    for counts, rows in calls:
        before = _lists(c)
        planned = c.plan(counts, final(rows))
        assert _lists(c) == before
        assert c.plan(counts, final(rows)) == planned
        out = c.advance(counts, final(rows))
        if kind == "sample":                    # (frames, pending before, padded)
            assert out[0] == planned and out[1] == before["pending"]
        elif kind == "rate":                    # (total before, emitted before, emitted by this call)
            assert out == (before["total"], before["emitted"], planned)
        else:                                   # (frames before, samples written by this call)
            assert out == planned and out[0] == before["emitted"]
        now = _lists(c)
        new = planned[1] if kind == "ola" else planned
        moved = "written" if kind == "ola" else "emitted"
        assert [a - b for a, b in zip(now[moved], before[moved])] == new
        assert now["ended"] == [e or b in rows for b, e in enumerate(before["ended"])]
    assert c.ended == [True, True, True]
