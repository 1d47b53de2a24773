"""GPU tests of STOI / ESTOI (csrc/stoi.hip, ops.stoi) against the float64 restatement tests/stoi_ref.py on the shared
inputs of that module: the smallest shapes that can still go wrong (one segment, none, every L mod 8 of the resampler, a
ragged batch with a row shorter than a frame, the committed 48100-sample pair).  These stop at 233 frames and 5 rows;
tests/test_stoi_long_gpu.py carries the same checks past 256 and 1024 frames and past 64 rows.

``info`` (frames, kept, segments) must equal the reference exactly -- every input has a margin of at least 0.01 dB, which
the test asserts of the reference alone -- and ``d`` must lie within stoi_ref.GPU_BOUND = 8 x the float32 stand-in's worst
error (2.4e-7) of the float64 score.  The 10 kHz cases take the resampler out, so a miss there is in the removal, the
transform or the segments.  Then the contracts: both = the two single calls bit for bit, a row alone = its bits in a batch,
run to run, row pitches, lengths with NaN behind them, and the drop-ins up to the evaluator's round trip."""
import os

import numpy as np
import pytest
import torch

import stoi_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_ = torch.tensor
NAN = float("nan")


def _ops():
    from avvad import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int64)


_ALONE = {}


def _alone(name):
    """(d (2,), info (3,)) of a case scored on its own with both=True, computed once"""
    if name not in _ALONE:
        fs, x, y = R.case(name)
        d, info = _ops().stoi(T_(x).to(DEV), T_(y).to(DEV), fs=fs, both=True, return_info=True)
        assert d.dtype == torch.float64 and d.shape == (1, 2) and info.dtype == torch.int32 and info.shape == (1, 3)
        _ALONE[name] = (d[0].clone(), info[0].clone())
    return _ALONE[name]


def _check(name, d, info, label=""):
    """margin, info exactly, |d - float64| <= GPU_BOUND: stoi_ref's checks, shared with the cases past one trip"""
    return R.check_scores(name, d.tolist(), info.tolist(), label)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_scores_and_info_against_float64(name):
    d, info = _alone(name)
    _check(name, d, info)
    if R.reference(name)["segments"] == 0:
        assert d.tolist() == [1e-5, 1e-5]


@pytest.mark.parametrize("name", ["k10_4097_one_segment", "k10_9001_half", "k16_9218", "k16_9731"])
def test_both_equals_the_single_calls_and_runs_repeat(name):
    ops = _ops()
    fs, x, y = R.case(name)
    xd, yd = T_(x).to(DEV), T_(y).to(DEV)
    d, info = _alone(name)
    s, si = ops.stoi(xd, yd, fs=fs, return_info=True)
    e, ei = ops.stoi(xd, yd, fs=fs, extended=True, return_info=True)
    assert s.shape == e.shape == (1,) and s.dtype == e.dtype == torch.float64
    assert torch.equal(_bits(s), _bits(d[:1])) and torch.equal(_bits(e), _bits(d[1:]))
    assert torch.equal(si[0], info) and torch.equal(ei[0], info)
    again = ops.stoi(xd, yd, fs=fs, both=True)
    assert torch.equal(_bits(again[0]), _bits(d))


def _batch(names, P, fill=NAN):
    """rows of pitch P holding the named cases (one rate), ``fill`` behind each row's length"""
    x = np.full((len(names), P), fill, dtype=np.float32)
    y = np.full((len(names), P), fill, dtype=np.float32)
    lengths = []
    for b, n in enumerate(names):
        _, cx, cy = R.case(n)
        x[b, :cx.size], y[b, :cx.size] = cx, cy
        lengths.append(cx.size)
    return T_(x).to(DEV), T_(y).to(DEV), lengths


@pytest.mark.parametrize("fs, names", [
    (10000, ["k10_9001_half", "k10_4097_one_segment", "short", "k10_4096_no_segment", "k10_6000_light"]),
    (16000, ["k16_16000_half", "k16_8705", "short", "k16_9731", "k16_11999"]),
])
def test_ragged_batch_rows_keep_their_bits(fs, names, lib_options):
    """B = 5 with a row shorter than a frame, NaN behind every length, a pitch wider than L: every row has the bits it has
    alone, also under a CU cap"""
    ops = _ops()
    real = [n for n in names if n != "short"]
    L = max(R.case(n)[1].size for n in real)
    P = L + 37
    x, y, lengths = _batch(real, P)
    at = names.index("short")
    x = torch.cat([x[:at], torch.full((1, P), NAN, device=DEV), x[at:]])
    y = torch.cat([y[:at], torch.full((1, P), NAN, device=DEV), y[at:]])
    x[at, :200], y[at, :200] = 0.1, 0.2
    lengths.insert(at, 200)
    for cap in (0, 24):
        lib_options("max_cus", cap)
        d, info = ops.stoi(x[:, :L], y[:, :L], lengths=lengths, fs=fs, both=True, return_info=True)
        assert d.shape == (5, 2) and info.shape == (5, 3)
        assert info[at].tolist() == [0, 0, 0] and d[at].tolist() == [1e-5, 1e-5]
        for b, n in enumerate(names):
            if n == "short":
                continue
            _check(n, d[b], info[b], "batch row %d (max_cus %d): " % (b, cap))
            da, ia = _alone(n)
            assert torch.equal(_bits(d[b]), _bits(da)) and torch.equal(info[b], ia)


def test_lengths_crop_and_planted_nan_is_not_read():
    """one signal, three lengths: each equals the cropped signal scored alone; without lengths the NaN arrives"""
    ops = _ops()
    fs, x, y = R.case("k16_11999")
    xd, yd = T_(x).to(DEV), T_(y).to(DEV)
    lens = [11999, 10244, 8192]
    xb, yb = xd.repeat(3, 1), yd.repeat(3, 1)
    for b, n in enumerate(lens):
        xb[b, n:], yb[b, n:] = NAN, NAN
    d, info = ops.stoi(xb, yb, lengths=torch.tensor(lens), fs=fs, both=True, return_info=True)
    for b, n in enumerate(lens):
        ref = R.score(x[:n], y[:n], fs)
        da, ia = ops.stoi(xd[:n], yd[:n], fs=fs, both=True, return_info=True)
        assert torch.equal(_bits(d[b]), _bits(da[0])) and torch.equal(info[b], ia[0])
        assert info[b].tolist() == [ref["frames"], ref["kept"], ref["segments"]]
        assert max(abs(float(d[b, 0]) - ref["stoi"]), abs(float(d[b, 1]) - ref["estoi"])) <= R.GPU_BOUND
    d_nan, info_nan = ops.stoi(xb[1:], yb[1:], fs=fs, both=True, return_info=True)
    assert info_nan[:, 1].tolist() == [0, 0] and d_nan.tolist() == [[1e-5, 1e-5]] * 2      # numpy's max of a NaN: nothing is kept


def test_metrics_drop_in_and_intelligibility_utt():
    from avvad import train as TR
    from packages import metrics
    fs, x, y = R.case("committed")
    x, y = x.copy(), y.copy()                                # (the drop-in hands its arrays to torch: writable ones)
    ref = R.reference("committed")
    got = metrics.stoi(x, y, fs), metrics.stoi(x, y, fs, extended=True)
    assert all(isinstance(v, float) for v in got)
    d, _ = _alone("committed")
    assert list(got) == d.tolist()
    fs10, x10, y10 = R.case("k10_9001_half")
    assert abs(metrics.stoi(x10.copy(), y10.copy(), fs_sig=10000) - R.reference("k10_9001_half")["stoi"]) <= R.GPU_BOUND
    with pytest.raises(ValueError, match="same length"):
        metrics.stoi(x, y[:-1])
    xd, yd = T_(x).to(DEV), T_(y).to(DEV)
    enhanced = 0.5 * (xd + yd)                               # halfway between the two: a stand-in for an enhanced signal
    s = TR.intelligibility_utt(enhanced, xd, yd)
    assert list(s) == list(TR.INTELLIGIBILITY_KEYS) == ["stoi", "estoi", "input_stoi", "input_estoi"]
    assert all(isinstance(v, float) for v in s.values())
    assert [s["input_stoi"], s["input_estoi"]] == d.tolist()
    want = R.score(x, enhanced.cpu().numpy(), fs)
    assert R.margin(x, fs) >= R.MIN_MARGIN_DB
    assert abs(s["stoi"] - want["stoi"]) <= R.GPU_BOUND and abs(s["estoi"] - want["estoi"]) <= R.GPU_BOUND
    assert abs(s["input_stoi"] - ref["stoi"]) <= R.GPU_BOUND and s["stoi"] > s["input_stoi"]


def _wav_pairs(tmp_path):
    from scipy.io import wavfile
    pairs = []
    for i in range(2):
        clean, noisy = R.speech_pair(70 + i, 9000, 16000, 5.0, 0.0)
        pc, pn = str(tmp_path / ("clean%d.wav" % i)), str(tmp_path / ("noisy%d.wav" % i))
        wavfile.write(pc, 16000, np.round(clean * 20000).astype(np.int16))
        wavfile.write(pn, 16000, np.round(noisy * 20000).astype(np.int16))
        pairs.append((pn, pc))
    return pairs


def test_evaluator_round_trip(tmp_path):
    from scipy.io import wavfile
    from avvad import train as TR
    from packages.models.Audio_Net import DeepVAD_audio
    pairs = _wav_pairs(tmp_path)
    make = lambda: DeepVAD_audio(1, 16, 513)                 # noqa: E731
    kw = dict(wav_list=[p[0] for p in pairs], clean_of=dict(pairs))
    out, wav, sc = (str(tmp_path / d) for d in ("out", "wav", "scores"))
    TR.evaluate_main("audio", make, out_dir=out, resynth_dir=wav, score_dir=sc, intelligibility=True, **kw)
    plain = {"tp", "tn", "fp", "fn"} | set(TR.SCORE_KEYS)
    for i, (pn, pc) in enumerate(pairs):
        d = torch.load(os.path.join(sc, "noisy%d_scores.pt" % i), weights_only=True)
        assert set(d) == plain | set(TR.INTELLIGIBILITY_KEYS)
        _, enhanced = wavfile.read(os.path.join(wav, "noisy%d_enhanced.wav" % i))
        noisy, clean = TR.load_waveform(pn)[0].numpy(), TR.load_waveform(pc)[0].numpy()
        assert R.margin(clean, 16000) >= R.MIN_MARGIN_DB
        e, x = R.score(clean, enhanced, 16000), R.score(clean, noisy, 16000)
        want = [e["stoi"], e["estoi"], x["stoi"], x["estoi"]]
        got = [d[k] for k in TR.INTELLIGIBILITY_KEYS]
        print("utterance %d: %s, float64 reference %s (segments %d)" % (i, got, want, e["segments"]))
        assert all(isinstance(v, float) for v in got) and e["segments"] > 0
        # the file holds intelligibility_utt of the three waveforms, bit for bit; the noisy input (this module's own kind of
        # signal) is held to the bound.  The enhanced signal is a hard mask of an untrained model: whole bands are window
        # leakage alone, the ill-conditioned input that stoi_ref.speech_pair describes (the float32 stand-in itself moves by
        # 4e-5 on such a signal), so it is held to the plumbing and to 1e-3, a check against gross errors only.
        ed, cd, xd = T_(enhanced).to(DEV), T_(clean).to(DEV), T_(noisy).to(DEV)
        assert TR.intelligibility_utt(ed, cd, xd) == {k: d[k] for k in TR.INTELLIGIBILITY_KEYS}
        assert np.abs(np.array(got[2:]) - np.array(want[2:])).max() <= R.GPU_BOUND
        assert np.abs(np.array(got[:2]) - np.array(want[:2])).max() <= 1e-3
    tables = TR.metrics_main(out, score_dir=sc, intelligibility=True)
    assert list(tables["enhancement"]["all"]) == list(TR.SCORE_KEYS) + list(TR.INTELLIGIBILITY_KEYS)
    assert list(TR.metrics_main(out, score_dir=sc)["enhancement"]["all"]) == list(TR.SCORE_KEYS)
    # the flags off: today's keys
    out0, wav0, sc0 = (str(tmp_path / d) for d in ("out0", "wav0", "scores0"))
    TR.evaluate_main("audio", make, out_dir=out0, resynth_dir=wav0, score_dir=sc0, **kw)
    for i in range(2):
        d0 = torch.load(os.path.join(sc0, "noisy%d_scores.pt" % i), weights_only=True)
        d1 = torch.load(os.path.join(sc, "noisy%d_scores.pt" % i), weights_only=True)
        assert set(d0) == plain and all(d0[k] == d1[k] for k in plain)
    with pytest.raises(SystemExit):
        TR.metrics_main(out0, score_dir=sc0, intelligibility=True)
    with pytest.raises(ValueError, match="resynth_dir and score_dir"):
        TR.evaluate_main("audio", make, out_dir=out0, score_dir=sc0, intelligibility=True, **kw)
