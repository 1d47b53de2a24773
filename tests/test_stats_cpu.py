"""CPU tests of the train-set statistics: the float64 restatement (tests/stats_ref.py) against a two-pass mean / std, the
reference's literal float32 accumulation against it, the file layout of ``Stats.save``, the host-side merge and rank
sharding, and the C ABI's validation of the new entry points (no device needed: they return before any launch).  For
test_stats_gpu.py's exact cases: the chunk and segment arithmetic of csrc/stats.hip restated (which branch each shape
reaches), a host model of the kernels that equals the plain sums, and its four mutants that do not."""
import ctypes as C
import os

import numpy as np
import torch

import stats_ref as R


def fixture_features():
    return [R.features64(x) for x in R.utterances()]


def test_restatement_equals_two_pass_statistics():
    feats = fixture_features()
    assert [f.shape for f in feats] == [(513, 185), (513, 185), (513, 115)]
    mean, std = R.stats64(feats)
    allx = np.concatenate(feats, axis=1)
    d_mean = np.abs(mean - allx.mean(axis=1)).max()
    d_std = np.abs(std - allx.std(axis=1, ddof=1)).max()
    print("restatement vs two-pass: mean %.2e std %.2e" % (d_mean, d_std))
    assert d_mean <= 1e-12 and d_std <= 1e-12


def test_reference_float32_accumulation_is_the_same_statistic():
    feats = fixture_features()
    mean, std = R.stats64(feats)
    m32, s32 = R.stats32_literal(feats)
    assert m32.dtype == np.float32 and s32.dtype == np.float32
    d_mean, d_std = np.abs(m32 - mean).max(), np.abs(s32 - std).max()
    print("reference float32 accumulation vs float64: mean %.2e std %.2e" % (d_mean, d_std))
    assert d_mean <= 1e-4 and d_std <= 1e-4


def test_stats_save_load_round_trip(tmp_path):
    from avvad.train import Stats
    rng = np.random.default_rng(3)
    am, asd = rng.standard_normal(513).astype(np.float32), rng.random(513).astype(np.float32) + 0.5
    vm, vs = np.float32([[0.37]]), np.float32([[0.21]])
    d = Stats(audio_mean=torch.from_numpy(am), audio_std=asd.reshape(-1, 1), video_mean=vm, video_std=vs).save(str(tmp_path / "m"))
    assert sorted(os.listdir(d)) == ["trainset_audio_mean.npy", "trainset_audio_std.npy", "trainset_video_mean.npy",
                                     "trainset_video_std.npy"]
    for name, want in (("audio_mean", am), ("audio_std", asd), ("video_mean", vm), ("video_std", vs)):
        got = np.load(os.path.join(d, "trainset_%s.npy" % name))
        assert got.dtype == np.float32 and got.shape == ((513, 1) if "audio" in name else (1, 1))
        assert np.array_equal(got.reshape(-1), want.reshape(-1))
    back = Stats.load(d)
    again = Stats.load(back.save(str(tmp_path / "m2")))
    for k, v in back._raw.items():
        assert np.array_equal(v, again._raw[k]) and v.dtype == again._raw[k].dtype
    only_audio = Stats(audio_mean=am, audio_std=asd).save(str(tmp_path / "a"))
    assert sorted(os.listdir(only_audio)) == ["trainset_audio_mean.npy", "trainset_audio_std.npy"]
    assert Stats.load(only_audio).get("video_mean", "cpu") is None


def test_merge_of_accumulators_equals_one_accumulation():
    from avvad.train import merge_stats
    feats = fixture_features()
    whole = R.accumulate(feats)
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        parts = [torch.from_numpy(R.accumulate([feats[i]])) for i in order]
        keep = [p.clone() for p in parts]
        merged = merge_stats(parts).numpy()
        assert all(torch.equal(p, k) for p, k in zip(parts, keep))           # inputs are left alone
        assert merged[-1] == whole[-1] == 485
        assert np.abs(merged - whole).max() <= 1e-12 * np.abs(whole).max()
        m, s = R.finalize(merged)
        m0, s0 = R.finalize(whole)
        assert np.abs(m - m0).max() <= 1e-12 and np.abs(s - s0).max() <= 1e-12
    two = merge_stats([torch.from_numpy(R.accumulate(feats[:2])), torch.from_numpy(R.accumulate(feats[2:]))]).numpy()
    assert np.abs(two - whole).max() <= 1e-12 * np.abs(whole).max()


def test_rank_sharding_covers_every_pair_once():
    from avvad.train import rank_shard
    for n in (0, 1, 5, 8, 17):
        for world in (1, 2, 3, 8):
            taken = sorted(i for r in range(world) for i in rank_shard(n, r, world))
            assert taken == list(range(n)), (n, world)


# ------------------------------------------------------------------------------------------ the oracles of test_stats_gpu.py
def test_exact_cases_reach_the_branches_they_are_named_for():
    br = {c[0]: R.branches(c[1], c[2], c[3], c[4], lengths=True if c[5] else None) for c in R.EXACT_CASES}
    assert br["one column, column form"]["form"] == "column" and br["one column, column form"]["lanes_in_last_block"] == 1
    assert br["one column, column form"]["boundaries_per_group"] == 8
    assert br["F 63: idle lane"]["col_blocks"] == 1 and br["F 63: idle lane"]["lanes_in_last_block"] == 63
    assert br["F 63: idle lane"]["boundaries_per_group"] == 3
    assert br["F 64: one full block"]["col_blocks"] == 1 and br["F 64: one full block"]["lanes_in_last_block"] == 64
    assert br["F 64: one full block"]["boundaries_per_group"] == 2
    assert br["F 65: one lane in block 2"]["col_blocks"] == 2 and br["F 65: one lane in block 2"]["lanes_in_last_block"] == 1
    assert br["F 65: one lane in block 2"]["nchunks"] == 3 and br["F 65: one lane in block 2"]["ragged_last_chunk"] == 297 - 256
    assert br["F 129: one lane in block 3"]["col_blocks"] == 3 and br["F 129: one lane in block 3"]["lanes_in_last_block"] == 1
    assert br["F 65 whole batch"]["count_trips"] == 0
    big = br["150 chunks + 37 rows"]
    assert big["nchunks"] == 151 and big["ragged_last_chunk"] == 37 and big["per"] == 10 >= R.ADD_UNROLL
    assert big["unrolled"] == [1] * 15 + [0] and big["remainder"] == [2] * 15 + [1]      # body in 15 segments, remainder in all 16
    assert big["count_trips"] == 19 and big["boundaries_per_group"] == 8
    # every case but the big one stays under eight chunks per segment: what the suite covered before it
    assert all(not any(v["unrolled"]) for k, v in br.items() if k != "150 chunks + 37 rows")
    # the fixture the existing tests use: 555 rows, 5 chunks, no eight-way body; a training set of ~370 chunks has one
    assert not any(R.branches(3, 185, 513, 513)["unrolled"]) and R.branches(370 * 128 - 5, 1, 513, 513)["per"] == 24
    for F, rows_per, nchunks, trips, idle in ((2, 8192, 1, 1, 254), (200, 81, 1, 1, 56), (5000, 3, 6, 20, 0), (16383, 1, 18, 64, 0),
                                              (16384, 1, 18, 64, 0), (20000, 1, 18, 79, 0)):
        b = br["scalar F %d" % F]
        assert b["form"] == "scalar" and (b["rows_per_chunk"], b["nchunks"], b["row_trips"], b["idle_lanes"]) == (rows_per, nchunks, trips, idle), F
    assert 16384 // 16383 == 1 and R.n_chunks(18, 16383, 1) == R.n_chunks(18, 16384, 1)          # the two sides of the F >= 16384 branch
    assert br["scalar count loop"]["count_trips"] == 2 and br["scalar count loop"]["form"] == "scalar"
    for name, B, T, F, nstat, ragged in R.EXACT_CASES:
        if ragged:
            lens = R.exact_case(name)[1]
            assert len(lens) == B and {0, T, T + 7, -2} <= set(lens), name


def test_model_of_the_kernels_is_exact_and_its_mutants_fail():
    """The host model of column_partials / scalar_partials / add_partials equals the plain float64 sums on every exact case;
    each planted mistake changes the result of the case that is there to catch it."""
    for name, B, T, F, nstat, ragged in R.EXACT_CASES:
        if F > 5000:
            continue                                             # the same scalar code path, only slower on the host
        x, lens, nstat = R.exact_case(name)
        want = R.host_sums(x, lens, nstat)
        assert want.max() < 2.0 ** 53 and np.array_equal(want, np.rint(want))
        assert np.array_equal(R.model_accumulate(x, lens, nstat), want), name
    x, lens, nstat = R.exact_case("150 chunks + 37 rows")
    want = R.host_sums(x, lens, nstat)
    for mutant in ("no_unroll", "drop_last_segment", "no_clamp", "no_t_reset"):
        assert not np.array_equal(R.model_accumulate(x, lens, nstat, mutant), want), mutant
    # the last segment of the big case is its ragged chunk alone
    assert np.array_equal(R.model_accumulate(x, lens, nstat, "drop_last_segment")[:-1],
                          R.host_sums(x[:150 * 128], lens[:150 * 128], nstat)[:-1])
    for name in ("F 63: idle lane", "F 64: one full block", "one column, column form"):      # several boundaries per group
        x, lens, nstat = R.exact_case(name)
        want = R.host_sums(x, lens, nstat)
        assert not np.array_equal(R.model_accumulate(x, lens, nstat, "no_t_reset")[:-1], want[:-1]), name
        assert R.model_accumulate(x, lens, nstat, "no_clamp")[-1] != want[-1], name
    x, lens, nstat = R.exact_case("scalar F 200")
    assert R.model_accumulate(x, lens, nstat, "no_clamp")[-1] != R.host_sums(x, lens, nstat)[-1]


def test_sum_bound_covers_two_orders_of_addition():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((700, 33)) * 18.0                   # full double mantissas: the order of the additions shows
    fwd = np.zeros(33)
    for row in x:
        fwd += row
    pair = x.reshape(2, 350, 33).sum(axis=1).sum(axis=0)
    b = R.sum_bound(x, 700)
    d = np.abs(fwd - pair)
    assert d.max() > 0 and np.all(d <= b) and np.all(b <= 1e-8) and np.all(b > 0)


def test_stats_entry_points_validate_before_any_launch():
    from avvad import _lib as L
    h = L.lib()
    ok = L.StftDesc(3, 48100, 1024, 256, 185, 1e-8)
    need = h.avvad_stft_stats_workspace(C.byref(ok))
    base = h.avvad_stft_workspace(C.byref(ok))
    chunks = (3 * 185 + 127) // 128
    assert base > 0 and need >= base + chunks * 2 * 513 * 8            # the spectrum stays live next to the partials
    assert h.avvad_stft_workspace(C.byref(ok)) == base                 # the STFT's own query is what it was
    for bad in (L.StftDesc(0, 48100, 1024, 256, 185, 1e-8), L.StftDesc(3, 48100, 1000, 256, 185, 1e-8),
                L.StftDesc(3, 48100, 1024, 0, 185, 1e-8), L.StftDesc(3, 48100, 1024, 256, 186, 1e-8)):
        assert h.avvad_stft_stats_workspace(C.byref(bad)) == 0
        assert h.avvad_stft_stats(0x1000, 0x1000, 0x1000, C.byref(bad), 0x1000, 1 << 40, None) == -1
    p = 0x1000                                                         # never dereferenced: every call below returns first
    assert h.avvad_stft_stats(None, p, p, C.byref(ok), p, need, None) == -1
    assert h.avvad_stft_stats(p, None, p, C.byref(ok), p, need, None) == -1
    assert h.avvad_stft_stats(p, p, None, C.byref(ok), p, need, None) == -1
    assert h.avvad_stft_stats(p, p, p, None, p, need, None) == -1
    assert h.avvad_stft_stats(p, p, p, C.byref(ok), None, need, None) == -1
    assert h.avvad_stft_stats(p, p, p, C.byref(ok), p, need - 1, None) == -2

    assert h.avvad_stats_workspace(485, 513) >= 4 * 2 * 513 * 8 and h.avvad_stats_workspace(20, 1) >= 20 * 2 * 8
    assert h.avvad_stats_workspace(0, 513) == 0 and h.avvad_stats_workspace(485, 0) == 0
    ws = h.avvad_stats_workspace(485, 513)
    assert h.avvad_stats_accumulate(None, None, p, 3, 185, 513, 513, p, ws, None) == -1
    assert h.avvad_stats_accumulate(p, None, None, 3, 185, 513, 513, p, ws, None) == -1
    assert h.avvad_stats_accumulate(p, None, p, 3, 185, 513, 513, None, ws, None) == -1
    assert h.avvad_stats_accumulate(p, None, p, 3, 185, 513, 2, p, ws, None) == -1        # nstat not in {1, F}
    assert h.avvad_stats_accumulate(p, None, p, 3, 185, 513, 0, p, ws, None) == -1
    assert h.avvad_stats_accumulate(p, None, p, 0, 185, 513, 513, p, ws, None) == -1
    assert h.avvad_stats_accumulate(p, None, p, 3, 0, 513, 513, p, ws, None) == -1
    assert h.avvad_stats_accumulate(p, None, p, 3, 185, 0, 1, p, ws, None) == -1
    assert h.avvad_stats_accumulate(p, None, p, 3, 185, 513, 513, p, ws - 1, None) == -2
    assert h.avvad_stats_finalize(None, 513, p, p, None) == -1
    assert h.avvad_stats_finalize(p, 513, None, p, None) == -1
    assert h.avvad_stats_finalize(p, 513, p, None, None) == -1
    assert h.avvad_stats_finalize(p, 0, p, p, None) == -1
