"""The resampler without a GPU: the float64 restatement of tests/resample_ref.py against scipy, its streamed form and the
host clock, the derived bound against stand-ins and mutants, the C ABI's symbols and refusals, and the host helpers of the
training layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import resample_ref as R
from conftest import ROOT

RATIOS9 = [(1, 3), (2, 1), (5, 8), (3, 1), (1, 6), (160, 441), (320, 441), (640, 441), (800, 999)]
NEW = ("avvad_resample_length", "avvad_resample_taps_len", "avvad_resample_hist", "avvad_resample", "avvad_resample_stream")


# ------------------------------------------------------------------------------------------------ restatement and taps
@pytest.mark.parametrize("up,down", RATIOS9)
def test_restatement_against_scipy(up, down):
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(up + 7 * down)
    for L in (1, 7, 100, 1001):
        x = rng.standard_normal(L)
        ref, A = R.resample(x, up, down)
        want = signal.resample_poly(x, up, down)
        assert len(ref) == len(want) == -(-L * up // down)
        assert float(np.abs(ref - want).max()) < 1e-13
        assert np.all(A >= np.abs(ref) * (1 - 1e-12))


@pytest.mark.parametrize("up,down", RATIOS9)
def test_taps_against_firwin_and_the_phase_major_layout(up, down):
    signal = pytest.importorskip("scipy.signal")
    from avvad import ops
    half, T, H = R.params(up, down)
    h = ops.resample_taps(up, down)
    assert h.dtype == np.float64 and h.shape == (2 * half + 1,) and np.array_equal(h, R.taps(up, down))
    want = up * signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0))
    assert float(np.abs(h - want).max()) < 1e-15 * up
    tp = ops.resample_taps_phase_major(up, down).reshape(up, T)
    for p in range(up):
        for j in range(T):
            assert tp[p, j] == (h[p + j * up] if p + j * up <= 2 * half else 0.0)


def test_five_eighths_is_the_stoi_table_bit_for_bit_and_lengths_are_ceil():
    from avvad import ops
    assert np.array_equal(ops.resample_taps(5, 8), ops.stoi_taps())
    for up, down in RATIOS9:
        for L in (0, 1, 2, 7, 440, 441, 442, 48000, 44100):
            assert ops.resample_length(L, up, down) == R.length(L, up, down) == int(np.ceil(L * up / down))


def test_resample_ratio():
    from avvad import ops
    from avvad._lib import AvvadError
    assert ops.resample_ratio(48000) == (1, 3) and ops.resample_ratio(44100) == (160, 441)
    assert ops.resample_ratio(19980) == (800, 999) and ops.resample_ratio(8000) == (2, 1)
    assert ops.resample_ratio(16000) == (1, 1) and ops.resample_ratio(16000, 10000) == (5, 8)
    for bad in ((0, 16000), (16000, -1), (44100.5, 16000), (16001, 16000), (True, 16000)):
        with pytest.raises(AvvadError, match="resample"):
            ops.resample_ratio(*bad)
    for bad in ((2, 4), (1, 1), (0, 3), (1025, 1)):
        with pytest.raises(AvvadError, match="%d/%d" % bad):
            ops.resample_taps(*bad)


# ------------------------------------------------------------------------------------------------ streaming and clock
SCHEDULES = [[1] * 300, [0, 1, 0, 0, 7, 441, 1, 0, 1000, 3, 0], [1451], [0, 0, 1, 0], [1000, 1, 0]]


@pytest.mark.parametrize("up,down", RATIOS9)
def test_streamed_restatement_equals_the_whole_one_and_holds_at_most_H(up, down):
    half, T, H = R.params(up, down)
    rng = np.random.default_rng(11)
    for packets in SCHEDULES:
        x = rng.standard_normal(sum(packets))
        ref, A = R.resample(x, up, down)
        got, gA, s = R.stream(x, packets, up, down)
        assert np.array_equal(got, ref) and np.array_equal(gA, A)
        assert s.held_max <= H - 2                                # H has two floats to spare


@pytest.mark.parametrize("up,down", [(1, 3), (160, 441), (2, 1), (800, 999)])
def test_rate_clock_against_the_emission_rule(up, down):
    from avvad.stream import RateClock
    from avvad._lib import AvvadError
    half, T, H = R.params(up, down)
    c = RateClock(2, up, down)
    for N in range(1, 2001):                                      # row 0 one sample at a time, row 1 idles
        before = c.emitted[0]
        plan = c.plan([1, 0])
        ib, ob, ne = c.advance([1, 0])
        a = N * up - 1 - half
        want = a // down + 1 if a >= 0 else 0
        assert c.count(N) == want == R.emitted(N, up, down)
        assert (ib, ob, ne) == ([N - 1, 0], [before, 0], [want - before, 0]) and plan == ne
        assert c.total == [N, 0] and c.emitted == [want, 0] and 0 <= c.pending[0] <= H - 2
    rnd = np.random.default_rng(5)
    c.reset()
    N = 0
    while N < 2000:                                               # packets of 0 .. 441
        n = int(rnd.integers(0, 442))
        N += n
        c.advance([n, 0])
        assert c.emitted[0] == R.emitted(N, up, down)
    ne = c.advance([3, 0], final=[0])[2]
    assert c.emitted[0] == R.length(N + 3, up, down) and ne[0] == c.emitted[0] - R.emitted(N, up, down) and c.ended == [True, False]
    with pytest.raises(AvvadError, match="reset"):
        c.plan([1, 0])
    with pytest.raises(AvvadError, match="reset"):
        c.advance([0, 0], final=[0])
    assert c.plan([0, 5]) == [0, c.count(5)]                      # an ended row may idle
    c.reset([0])
    assert c.total[0] == c.emitted[0] == c.pending[0] == 0 and c.plan([1, 0]) == [c.count(1), 0]
    for bad in ([1], [-1, 0]):
        with pytest.raises(AvvadError):
            c.plan(bad)
    c.preset(1, 3_000_000_000)
    assert c.emitted[1] == R.emitted(3_000_000_000, up, down) and c.pending[1] <= H - 2
    with pytest.raises(AvvadError):
        RateClock(1, 2, 4)


# ------------------------------------------------------------------------------------------------ stand-ins and mutants
def _standin(x, up, down, n0, n1, pos0=0, first=0, last=None, acc=np.float64, scale=True, centre=0, phase=0, wrap32=False):
    """A kernel stand-in on the host: the chain of the definition, one product and one addition at a time in ``acc``,
    rounded to float32 at the end.  The knobs are the mutants: ``scale`` False leaves the taps without their factor up,
    ``centre`` moves the filter's centre, ``phase`` the tap index, ``wrap32`` forms n * down in 32 bits."""
    half = R.params(up, down)[0]
    h = R.taps(up, down)
    if not scale:
        h = h / up
    last = pos0 + len(x) - 1 if last is None else last
    out = np.zeros(max(n1 - n0, 0), dtype=np.float32)
    for i, n in enumerate(range(n0, n1)):
        nd = n * down
        if wrap32:
            nd = (nd + 2 ** 31) % 2 ** 32 - 2 ** 31
        q = nd + half + centre
        lo, hi = max(first, -((2 * half - q) // up)), min(last, q // up)
        s = acc(0.0)
        for m in range(lo, hi + 1):
            t = q - m * up + phase
            if 0 <= t <= 2 * half:
                s = acc(s + acc(acc(h[t]) * acc(x[m - pos0])))
        out[i] = np.float32(s)
    return out


def _exceeds(got, ref, A, up, down):
    """fraction of the outputs beyond the bound, and the largest error in units of it"""
    err, tol = np.abs(got.astype(np.float64) - ref), R.tol(ref, A, up, down)
    return float(np.mean(err > tol)), float((err / tol).max())


CASES = [(1, 3, 400), (160, 441, 900), (2, 1, 150), (800, 999, 500)]


@pytest.mark.parametrize("up,down,L", CASES)
def test_the_double_standin_is_within_the_bound(up, down, L):
    x = np.random.default_rng(3).standard_normal(L).astype(np.float32)
    ref, A = R.resample(x, up, down)
    frac, worst = _exceeds(_standin(x, up, down, 0, len(ref)), ref, A, up, down)
    assert frac == 0.0 and worst <= 1.0


MUTANTS = ["float32 accumulation", "taps not scaled by up", "centre + 1", "centre - 1", "phase + 1", "phase - 1"]


@pytest.mark.parametrize("up,down,L,mutant", [c + (m,) for c in CASES for m in MUTANTS
                                              if not (m == "taps not scaled by up" and c[0] == 1)])    # (at up = 1 the factor is 1)
def test_value_mutants_are_rejected(up, down, L, mutant):
    x = np.random.default_rng(3).standard_normal(L).astype(np.float32)
    ref, A = R.resample(x, up, down)
    kw = {"float32 accumulation": dict(acc=np.float32), "taps not scaled by up": dict(scale=False), "centre + 1": dict(centre=1),
          "centre - 1": dict(centre=-1), "phase + 1": dict(phase=1), "phase - 1": dict(phase=-1)}[mutant]
    frac, worst = _exceeds(_standin(x, up, down, 0, len(ref), **kw), ref, A, up, down)
    assert frac > 0.2 and worst > 10, (frac, worst)


def test_count_and_state_mutants_are_rejected():
    """``floor`` for the length and a stream whose last call is not final lose outputs; a history short of the T - 1
    inputs an output can need behind the newest (the state's H has two more) loses terms.  The mutant keeps T - 3: at up = 1
    the outermost tap sits on a zero crossing of the sinc (1e-17), so the first term whose loss shows is the next one."""
    from avvad import ops
    x = np.random.default_rng(9).standard_normal(1001)
    for up, down in ((1, 3), (160, 441), (5, 8)):
        half, T, H = R.params(up, down)
        ref, A = R.resample(x, up, down)
        assert len(ref) == ops.resample_length(len(x), up, down) != len(x) * up // down          # floor is one short
        got, _, _ = R.stream(x, [500, 501], up, down, final=False)
        assert len(got) == R.emitted(len(x), up, down) < len(ref)                                 # final not flushed
        ok, _, _ = R.stream(x, [1] * 1001, up, down, hist=T - 1)
        assert np.array_equal(ok, ref)
        short, _, _ = R.stream(x, [1] * 1001, up, down, hist=T - 3)
        frac, worst = _exceeds(short.astype(np.float32), ref, A, up, down)
        assert frac > 0.0 and worst > 10, (up, down, frac, worst)


def test_thirty_two_bit_positions_are_rejected_at_three_billion():
    start = 3_000_000_000
    x = np.random.default_rng(2).standard_normal(300).astype(np.float32)
    for up, down in ((1, 3), (160, 441)):
        H = R.params(up, down)[2]
        ref, A, _ = R.stream(x, [300], up, down, start=start)
        n0 = R.emitted(start, up, down)
        hist = np.concatenate([np.zeros(H, dtype=np.float32), x])
        args = (hist, up, down, n0, n0 + len(ref), start - H, start - H, start + len(x) - 1)
        assert _exceeds(_standin(*args), ref, A, up, down)[0] == 0.0
        frac, worst = _exceeds(_standin(*args, wrap32=True), ref, A, up, down)
        assert frac > 0.5 and worst > 10


# ------------------------------------------------------------------------------------------------ symbols and refusals
def test_symbols_are_declared_bound_and_exported():
    from avvad import _lib as L
    h = L.lib()
    assert h.avvad_abi_version() == L.ABI_VERSION == 3            # added entry points change no signature
    header = open(os.path.join(ROOT, "include", "avvad.h")).read()
    assert int(re.search(r"#define AVVAD_ABI_VERSION (\d+)", header).group(1)) == 3
    declared = set(re.findall(r"\b(avvad_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(h, name), name
    build = open(os.path.join(ROOT, "audio-visual-vad_amd", "csrc", "build.sh")).read()
    assert re.search(r'SRCS="[^"]*\bresample\b[^"]*"', build)
    assert int(re.search(r"#define AVVAD_RESAMPLE_TILE (\d+)", header).group(1)) == L.RESAMPLE_TILE
    assert int(re.search(r"#define AVVAD_RESAMPLE_MAX_RATE (\d+)", header).group(1)) == L.RESAMPLE_MAX_RATE == 1024


def test_queries():
    from avvad import _lib as L, ops
    h = L.lib()
    for up, down in RATIOS9:
        half, T, H = R.params(up, down)
        assert h.avvad_resample_hist(up, down) == H and h.avvad_resample_taps_len(up, down) == up * T
        assert len(ops.resample_taps_phase_major(up, down)) == up * T
        for n in (0, 1, 999, 48000):
            assert h.avvad_resample_length(n, up, down) == R.length(n, up, down)
    for bad in ((0, 1), (1, 0), (2, 4), (1, 1), (1025, 1), (1, 1025), (-3, 2)):
        assert h.avvad_resample_hist(*bad) == h.avvad_resample_taps_len(*bad) == h.avvad_resample_length(10, *bad) == 0
    assert h.avvad_resample_length(-1, 1, 3) == 0


def _host(n, fill=7.25):
    a = np.full(n, fill, dtype=np.float32)
    return a, C.c_void_p(a.ctypes.data)


def test_refusals_need_no_gpu_and_leave_the_output_alone():
    """Every refused call returns before anything is launched: the buffers here are host memory with a pattern, the pointers
    are never dereferenced, and the pattern is whole afterwards."""
    from avvad import _lib as L
    h = L.lib()
    p = lambda v: C.c_void_p(v)                              # noqa: E731
    Lx, up, down = 90, 1, 3
    out, outp = _host(64)
    #      x         ld  lengths taps     up  down out   ld  n_out B  L   stream
    ok = [p(0x1000), Lx, None, p(0x2000), up, down, outp, 30, None, 1, Lx, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return h.avvad_resample(*a)
    for i in (0, 3, 6):                                       # a NULL where a buffer is needed
        assert call(**{"a%d" % i: None}) == -1, i
    assert call(a4=0) == call(a5=0) == call(a4=-1) == -1     # up or down < 1
    assert call(a4=2, a5=4) == call(a4=3, a5=3) == -1        # not in lowest terms
    assert call(a4=1, a5=1) == -1                            # 1/1 passes through in the Python layer
    assert call(a4=1025, a5=1) == call(a4=1, a5=1025) == -1
    assert call(a9=0) == call(a9=65536) == call(a10=0) == -1
    assert call(a1=Lx - 1) == call(a7=29) == -1              # a pitch below its row
    assert call(a3=p(0x2004)) == -1                          # taps off their 8 bytes
    assert np.all(out == 7.25)

    H = R.params(up, down)[2]
    st, stp = _host(2 * H)
    #      chunk     ld  n_valid    in_before  out_before n_emit     state_in   state_out taps    up  down  out  ld  B  n_in n_max stream
    ok2 = [p(0x1000), 50, p(0x3000), p(0x4000), p(0x5000), p(0x6000), p(0x7000), stp, p(0x2000), up, down, outp, 20, 2, 50, 20, None]

    def call2(**kw):
        a = list(ok2)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return h.avvad_resample_stream(*a)
    for i in (0, 2, 3, 4, 5, 6, 7, 8, 11):
        assert call2(**{"a%d" % i: None}) == -1, i
    assert call2(a9=0) == call2(a10=0) == call2(a9=2, a10=4) == call2(a9=1, a10=1) == call2(a9=1025, a10=1) == -1
    assert call2(a13=0) == call2(a13=65536) == call2(a14=-1) == call2(a15=-1) == -1
    assert call2(a1=49) == call2(a12=19) == -1
    assert call2(a8=p(0x2004)) == -1
    assert call2(a6=stp) == -1                               # state_in == state_out
    assert np.all(out == 7.25) and np.all(st == 7.25)


# ------------------------------------------------------------------------------------------------ the training layer's host side
def _npz(path, n, fs, seed=0):
    x = (np.random.default_rng(seed).standard_normal(n) * 3000).astype(np.int16)
    np.savez(path, samples=x, fs=fs)
    return str(path)


def test_to_16k_groups_by_rate_and_keeps_the_order(monkeypatch):
    from avvad import ops, train as TR
    calls = []

    def fake(wave, lengths=None, fs_in=None, fs_out=16000):
        calls.append((fs_in, tuple(wave.shape), list(lengths)))
        n = [-(-k * 16000 // fs_in) for k in lengths]
        out = torch.zeros(wave.shape[0], -(-wave.shape[1] * 16000 // fs_in))
        for b, k in enumerate(n):
            out[b, :k] = fs_in + wave[b, 0]                       # a mark of the row it came from
        return out, n
    monkeypatch.setattr(ops, "resample", fake)
    lens, rates = [30, 12, 48, 16, 9], [48000, 16000, 48000, 8000, 16000]
    w = torch.zeros(5, 48)
    for b, n in enumerate(lens):
        w[b, :n] = b + 1
    out, n16 = TR.to_16k(w, torch.LongTensor(lens), torch.LongTensor(rates), "cpu")
    assert calls == [(48000, (2, 48), [30, 48]), (8000, (1, 16), [16])]        # one call per rate other than 16 kHz
    assert n16 == [10, 12, 16, 32, 9] and out.shape == (5, 32)
    for b, want in enumerate([48001.0, 2.0, 48003.0, 8004.0, 5.0]):
        assert torch.all(out[b, :n16[b]] == want) and torch.all(out[b, n16[b]:] == 0), b
    calls.clear()
    out, n16 = TR.to_16k(w, lens, [16000] * 5, "cpu")                          # nothing to resample: the rows as they are
    assert not calls and n16 == lens and torch.equal(out, w)
    with pytest.raises(ValueError):
        TR.to_16k(w, lens, rates[:4], "cpu")


def test_collates_carry_rates_only_when_the_items_do(tmp_path):
    from avvad import train as TR
    a, b = _npz(tmp_path / "a.npz", 480, 48000, 1), _npz(tmp_path / "b.npz", 200, 16000, 2)
    ds = TR.CleanWavs([a, b], resample=True)
    lens, clean, rates = TR.CleanWavs.collate([ds[0], ds[1]])
    assert lens.tolist() == [480, 200] and rates.tolist() == [48000, 16000] and clean.shape == (2, 480)
    assert len(TR.CleanWavs.collate([TR.CleanWavs([b])[0]])) == 2
    pairs = TR.WavPairs([(a, b), (b, b)], resample=True)
    lens, noisy, clean, rates = TR.WavPairs.collate([pairs[0], pairs[1]])
    assert lens.tolist() == [[480, 200], [200, 200]] and rates.tolist() == [[48000, 16000], [16000, 16000]]
    assert noisy.shape == (2, 480) and clean.shape == (2, 200)
    assert len(TR.WavPairs.collate([TR.WavPairs([(b, b)])[0]])) == 3


def test_other_rates_are_still_refused_by_default(tmp_path):
    from avvad import train as TR
    a, b = _npz(tmp_path / "a.npz", 480, 48000, 1), _npz(tmp_path / "b.npz", 200, 16000, 2)
    with pytest.raises(ValueError, match="expected 16 kHz audio, got 48000"):
        TR.CleanWavs([a])[0]
    with pytest.raises(ValueError, match="expected 16 kHz audio"):
        TR.WavPairs([(b, a)])[0]
    with pytest.raises(ValueError, match="expected 16 kHz audio, got 48000"):
        TR.read_noise_bank([b, a], "cpu")
    with pytest.raises(ValueError, match="expected 16 kHz audio, got 48000"):
        TR.clean_vad_labels(a, 100, "cpu")
    with pytest.raises(ValueError, match="expected 16 kHz audio, got 48000"):
        TR.load_16k(a, "cpu")
