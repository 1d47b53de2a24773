"""CPU tests of the streaming STFT oracle (tests/stft_stream_ref.py): the lines of csrc/stream_product.h and
csrc/stft_stream.hip its restatements cite, the restated plan against what every case declares it reaches, the clamp rule
against a transliteration of ``ss_row``, the streamed framing against the whole-utterance framing, the unchecked shares on the
reference alone, the n_fft limit through the library's host side, every case of tests/test_stft_stream_kernels_gpu.py with the
float32 twin in the place of the HIP path, and mutants of that twin which the assertion named for each must reject."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import stft_ref as R
import stft_stream_ref as S

TAG = "cpu32"
TWIN = S.make_twin()
CACHE = {}


def _src(name):
    with open(os.path.join(S.CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------ the restatements against the source
def test_cited_lines_hold():
    lines = {f: _src(f).split("\n") for f in {c[0] for c in S.CITES}}
    for f, n, text in S.CITES:
        assert text in lines[f][n - 1], "%s:%d no longer holds %r: move the citation in stft_stream_ref" % (f, n, text)
    assert (S.NW, S.PAD, S.LDS_MAX, S.K_MAX, S.SS_SLOT_INTS) == (512 // 64, 4, 150 * 1024, 2048, 5)


def test_plan_restated_and_its_boundary_sizes():
    """1184 is the largest n_fft that runs two frame groups, 1216 the first that falls back to one, 2368 the largest the plan
    itself takes -- which is why the descriptor check enforces the documented 2048"""
    two = [n for n in range(32, 4097, 32) if S.plan(n, 2, S.SS_SLOT_INTS, 17)["NG"] == 2]
    one = [n for n in range(32, 4097, 32) if S.plan(n, 2, S.SS_SLOT_INTS, 17)["NG"] == 1]
    assert max(two) == 1184 and min(one) == 1216 and max(one) == 2368
    assert max(n for n in range(32, 4097, 32) if S.plan(n, 1, 2, 1)["NG"]) == 2368        # the inverse's single plane: the same limit
    assert S.plan(1184, 2, 5, 17)["lds"] <= S.LDS_MAX < S.lds_bytes(1216, 2, 5, 2)[0]
    assert S.plan(1024, 2, 5, 16) == dict(NG=1, ny=1, lds=16 * 1028 * 4 + 336)
    assert S.plan(1024, 2, 5, 17)["ny"] == 1 and S.plan(1024, 2, 5, 33)["ny"] == 2 and S.plan(32, 2, 5, 10 ** 6)["ny"] == 16
    assert S.plan(32, 2, 5, 17)["lds"] == 2 * 2 * 8 * 64 * 16 + 656                       # the partial sums outgrow the frames
    # the operand permutation is one: every k of a frame exactly once
    for K in (32, 96, 160, 1024):
        ks = sorted(S.operand_index(K, kk, q, j) for kk in range(K // 16) for q in range(4) for j in range(4))
        assert ks == list(range(K))


@pytest.mark.parametrize("name", [n for n, c in S.CASES.items() if c["reach"]])
def test_cases_reach_what_they_declare(name):
    c = S.CASES[name]
    got = S.case_reach(name, c["policies"][0])
    for k, v in c["reach"].items():
        assert got[k] == v, (name, k, got[k], v)


def test_the_cases_reach_every_path_together():
    reach = {(n, p): S.case_reach(n, p) for n, c in S.CASES.items() for p in c["policies"]}
    assert {n for (n, p) in S.IMPULSE} >= {"imp-%dx%d-%s" % (a, b, w) for a, b in S.CONFIGS for w in ("minus", "exact", "plus")}
    assert any(r["idle_waves"] == 6 for r in reach.values()) and any(r["idle_waves"] == 2 for r in reach.values())
    assert reach[("imp-160x48-exact", "one")]["uneven"] and S.CASES["imp-160x48-exact"]["n_fft"] // 16 == 10
    r = reach[("round-1184x296-B2", "one")]
    assert r["NG"] == 2 and r["lds"] == 152720 <= S.LDS_MAX                               # NG = 2 at its LDS limit
    for n in ("fallback-1216", "max-2048", "round-1216x304-B2", "round-2048x512-B2"):
        assert reach[(n, "one")]["NG"] == 1 and reach[(n, "one")]["per_call"][0] > 16      # NG = 1 forced, more than 16 frames
    assert reach[("many-32x1", "one")]["per_call"][0] > 16 * 32 and reach[("many-32x1", "one")]["trips"] == 2
    r = reach[("rows-130", "one")]
    assert r["row_groups"] == 3 and r["rows_over_tail_wgs"] and r["rows_in_pass"] > 1
    q = S.RAGGED_POLICY_REACH
    assert reach[(q["name"], q["policy"])]["rows_over_fill_slots"] and reach[(q["name"], q["policy"])]["rows_over_tail_wgs"]
    assert reach[("ng-edge", "edge")]["per_call"] == [16, 17, 32, 33]
    lens = S.CASES["rows-130"]["lengths"]
    assert len(lens) == 130 and all(S.frames_total(lens[b], 32, 8) == 0 for b in (3, 63, 64, 65, 127, 128)) and lens[64] and lens[127]
    # the direct scenario: 21 frames, so d->M = 1 walks NG = 1 over more than 16; the policies stay within a few hundred calls
    assert sum(S.direct_scenario(96, 32)["n_frames"]) == 21 and S.plan(96, 2, 5, 1) == dict(NG=1, ny=1, lds=2 * 8 * 64 * 16 + 336)
    assert max(len(S.case_calls(n, p)) for n, c in S.CASES.items() for p in c["policies"]) <= 301
    rag = S.case_calls("imp-96x32-plus", "ragged")
    assert any(0 in n for n, _ in rag) and len({i for i, (_, fin) in enumerate(rag) if fin}) > 1   # zero-sample calls; rows end apart


def test_clamp_rule_agrees_with_ss_row():
    """``clamped_counts`` against a line-by-line transliteration of ss_row (stft_stream.hip lines 56 .. 62, cited) on counts that
    are wrong in every direction"""
    rng = np.random.default_rng(4)
    cc = lambda v, hi: 0 if v < 0 else (hi if v > hi else v)
    for _ in range(2000):
        K = int(rng.choice([32, 96, 1024]))
        hop, L, T = int(rng.integers(1, K + 1)), int(rng.integers(1, 3 * K)), int(rng.integers(0, 9))
        nvi, npi, nfi, pad = int(rng.integers(-5, L + 6)), int(rng.integers(-5, K + 6)), int(rng.integers(-3, 12)), int(rng.integers(0, 2))
        call = S.make_call(dict(n_fft=K, hop=hop), np.zeros((1, L)), [nvi], [npi], [nfi], [pad], np.zeros((1, K)), T=T)
        nv, npd = cc(nvi, L), cc(npi, K)
        Ls = nv + npd
        cap = ((Ls - K) // hop + 1 if Ls >= K else 0) + (1 if pad else 0)
        if cap > T:
            cap = T
        assert S.clamped_counts(call) == [(nv, npd, cc(nfi, cap))]
        r = S.ref_call(call)
        assert r["frames"][0].shape == (cc(nfi, cap), K) and r["state"].shape == (1, K)


@pytest.mark.parametrize("name,policy", [("imp-160x48-minus", "hop"), ("imp-32x1-plus", "ragged"), ("round-96x32-feat", "hop"),
                                         ("imp-1024x1024-exact", "ragged")])
def test_streamed_framing_is_the_whole_utterance_framing(name, policy):
    """the restated stream alone: whatever the split, the frames a row's calls gather are ``stft_ref.frames_of`` of its wave,
    bit for bit, and ``hop = n_fft`` leaves no tail behind a complete frame"""
    c = S.CASES[name]
    x = np.random.default_rng(1).standard_normal((c["B"], c["L"])).astype(np.float32)
    quiet = lambda call: dict(out=np.zeros((c["B"], call["T"], c["n_fft"] // 2 + 1), np.float32),
                              spec=np.zeros((c["B"], call["T"], c["n_fft"] // 2 + 1, 2), np.float32), state=S.ref_call(call)["state"])
    res = S.stream_through(quiet, name, S.cfg_of(c), list(x), S.case_calls(name, policy))
    T = S.frames_total(c["L"], c["n_fft"], c["hop"])
    want = R.frames_of(x, c["n_fft"], c["hop"], T).reshape(c["B"], T, -1)
    for b in range(c["B"]):
        assert np.array_equal(S.bits(res["frames"][b]), S.bits(want[b])), (name, b)
    assert [sum(nf) for nf in res["n_frames"]] == [sum(nf) for nf in S.case_frames_per_call(name, policy)]


@pytest.mark.parametrize("name", sorted({n for n, _ in S.FEATURES}))
def test_unchecked_shares_on_the_reference_alone(name):
    share = S.unchecked_share(name)
    assert share <= S.CASES[name]["unchecked_max"], (name, share)
    if S.CASES[name]["base"]:
        assert share == R.unchecked_share(name)                                           # stft_ref's own reference
    assert S.CASES["feat-32x8-peak3.7"]["unchecked_max"] == 0.0 and not S._pow2(3.7) and S._pow2(2.0) and S._pow2(0.25)


def test_required_impulse_positions():
    """sample 0 and L - 1, both sides of every call boundary, the straddling frames' ends, the pad frame's predecessor"""
    name, policy = "imp-1024x256-minus", "hop"
    c = S.CASES[name]
    need = S.required_positions(name, policy)[0]
    L, T = c["L"], S.frames_total(c["L"], 1024, 256)
    assert T == 8 and {0, L - 1, (T - 2) * 256 + 1023} <= set(need)
    for k in range(1, L // 256 + 1):
        assert {256 * k - 1, 256 * k} <= set(need), k
    assert {256, 1279, 512, 1535} <= set(need)                                            # frames 1 and 2 straddle the calls after 1024 and 1280 samples
    placed = [sorted(p for w in S.impulse_waves(name, policy) for p, _ in w[1][b]) for b in range(3)]
    assert all(set(need) <= set(pl) for pl in placed)
    for rows, pl in S.impulse_waves(name, policy):
        for b in range(3):
            ps = sorted(p for p, _ in pl[b])
            assert all(q - p >= 1024 for p, q in zip(ps, ps[1:])) and np.count_nonzero(rows[b]) == len(ps)


# ------------------------------------------------------------------------------------------ the n_fft limit, host side only
def test_the_documented_n_fft_limit_is_enforced():
    """include/avvad.h: n_fft <= 2048 for both streaming transforms; the product's plan alone would take 2368.  2048 is
    accepted by the size queries, 2080 is AVVAD_EINVAL before anything is launched (the pointers are never dereferenced)."""
    from avvad import _lib as L
    h = L.lib()
    assert h.avvad_stft_stream_basis_bytes(2048) == 65 * 2 * 16 * 2048 * 4 and h.avvad_istft_stream_basis_bytes(2048) > 0
    for n in (2080, 2368, 2400):
        assert h.avvad_stft_stream_basis_bytes(n) == 0 and h.avvad_istft_stream_basis_bytes(n) == 0
    one, two = C.c_void_p(64), C.c_void_p(128)
    args = [one, one, one, one, one, None, one, two, one, None, None, one]
    assert h.avvad_stft_stream_fwd(*args, C.byref(L.StftStreamDesc(2, 256, 2080, 256, 1, 2, 1e-8, 1e-8)), None) == -1
    assert h.avvad_stft_stream_fwd_spec(*args, one, C.byref(L.StftStreamDesc(2, 256, 2080, 256, 1, 2, 1e-8, 1e-8)), None) == -1
    assert h.avvad_stft_stream_basis(2080, one, None) == -1 and h.avvad_istft_stream_basis(2080, one, None) == -1
    assert h.avvad_istft_stream_workspace(C.byref(L.IstftStreamDesc(2, 3, 2080, 256, 768, 5, 1))) == 0
    assert h.avvad_istft_stream_workspace(C.byref(L.IstftStreamDesc(2, 3, 2048, 256, 768, 5, 1))) > 0
    header = open(os.path.join(os.path.dirname(S.CSRC), "..", "include", "avvad.h")).read()
    assert len(re.findall(r"n_fft <= 2048", header)) == 2


# ------------------------------------------------------------------------------------------ the twin passes every tier
COUNT = [0, 0]


@pytest.mark.parametrize("name,policy", S.IMPULSE + S.GRID)
def test_twin_impulse_tier(name, policy):
    off, total = S.check_impulse(TWIN, name, policy, tag=TAG)
    assert off == 0 and total > 0                                                         # the twin's basis IS float32(reference)
    COUNT[0], COUNT[1] = COUNT[0] + off, COUNT[1] + total


@pytest.mark.parametrize("name,policy", S.ROUNDING)
def test_twin_rounding_tier(name, policy):
    fig = S.check_rounding(TWIN, name, policy, tag=TAG, cache=CACHE)
    assert 0 < fig["worst"] < 0.1
    if policy == "one":                                                                   # and as one sequential chain
        S.check_rounding(S.make_twin(order="chain"), name, policy, tag="chain")


@pytest.mark.parametrize("name,policy", S.FEATURES)
def test_twin_feature_tier(name, policy):
    S.check_features(TWIN, name, policy, tag=TAG, cache=CACHE)


@pytest.mark.parametrize("name,policy", S.SILENCE)
def test_twin_silence(name, policy):
    S.check_silence(TWIN, name, policy)


@pytest.mark.parametrize("n_fft,hop", S.DIRECT)
def test_twin_direct_calls_and_clamping(n_fft, hop):
    S.check_direct(TWIN, n_fft, hop, tag=TAG)
    for v in S.CLAMP_VARIANTS:
        r = S.check_clamp(TWIN, n_fft, hop, v, tag=TAG)
        honest = S.direct_scenario(n_fft, hop, seed=1)["n_frames"]
        got = [c[2] for c in r["counts"]]
        assert got == {"pending+2": [honest[0] + 1] + honest[1:], "negative": [0, honest[1], 1],
                       "pad-frames+1": [honest[0], honest[1] + 1, honest[2]]}.get(v, honest), (v, got)


# ------------------------------------------------------------------------------------------ every assertion can fail
def _run(mutant, kind, a, b):
    tw = S.make_twin(mutant)
    if kind == "impulse":
        S.check_impulse(tw, a, b, tag=None)
    elif kind == "rounding":
        S.check_rounding(tw, a, b, tag=None)
    elif kind == "features":
        S.check_features(tw, a, b, tag=None)
    else:
        assert kind == "clamp"
        S.check_clamp(tw, a, dict(S.DIRECT)[a], b, tag=None)


MUTANT_FAILS = [
    ("tail_late", "state", "impulse", "imp-32x8-exact", "hop"),
    ("ignore_pending", "spectrum", "impulse", "imp-1024x256-exact", "hop"),
    ("pad_reads_behind", "zero", "impulse", "imp-96x32-minus", "one"),
    ("pad_not_final", "clamp", "clamp", 96, "frames+1+2"),
    ("peak_multiplies", "spectrum", "rounding", "round-256x64-B3", "one"),
    ("peak_multiplies", "spectrum", "features", "feat-32x8-peak3.7", "one"),
    ("no_scan_base", "zero", "impulse", "rows-130", "one"),
    ("skip_last_group", "spectrum", "impulse", "imp-160x48-exact", "hop"),
    ("skip_last_group", "spectrum", "rounding", "round-160x48-B2", "one"),
    ("last_bin_unwritten", "zero", "impulse", "imp-32x8-exact", "one"),
    ("no_zero_fill", "zero-fill", "impulse", "imp-96x32-plus", "ragged"),
    ("no_zero_fill", "zero-fill", "impulse", "rows-130", "one"),
    ("idle_rewritten", "state", "impulse", "imp-96x32-plus", "ragged"),
    ("nvalid_unclamped", "clamp", "clamp", 96, "valid+3"),
    ("nvalid_unclamped", "clamp", "clamp", 1024, "valid+3"),
    ("f32_trig", "zero", "rounding", "round-1024x256-B3", "one"),
    ("f32_trig_zeros", "aggregate", "rounding", "round-1024x256-B3", "one"),
    ("f32_trig_zeros", "aggregate", "rounding", "round-96x32-B3", "one"),
    ("f32_trig_zeros", "aggregate", "rounding", "round-2048x512-B2", "one"),
    ("imag_sign", "spectrum", "impulse", "imp-32x8-exact", "one"),
    ("bf16_operands", "spectrum", "rounding", "round-1024x256-B3", "one"),
    ("no_norm_eps", "standardised", "features", "round-32x8-feat", "one"),
]


@pytest.mark.parametrize("mutant,tag,kind,a,b", MUTANT_FAILS)
def test_mutants_fail_where_declared(mutant, tag, kind, a, b):
    with pytest.raises(AssertionError, match=r"^\[%s\]" % re.escape(tag)):
        _run(mutant, kind, a, b)


def test_every_mutant_is_declared():
    assert {m[0] for m in MUTANT_FAILS} == set(S.MUTANTS)


def test_the_remaining_assertions_can_fail():
    """[guard], [hint-bits], [pitch], [peak-bits], [same-bits], [split-bits]: implementations that are wrong in just that way"""
    def guarded(call):
        g = TWIN(call)
        g["guards"] = [("behind out", False)] if call["arena"] else []
        return g
    with pytest.raises(AssertionError, match=r"^\[guard\]"):
        S.check_clamp(guarded, 96, 32, "negative", tag=None)

    def twisted(when):
        def impl(call):
            g = TWIN(call)
            if when(call):
                g["out"] = np.nextafter(g["out"], np.float32(np.inf))
            return g
        return impl
    total = sum(S.direct_scenario(96, 32)["n_frames"])
    for tag, when in (("hint-bits", lambda c: c["M"] == 1), ("pitch", lambda c: c["T"] == 10), ("peak-bits", lambda c: c["peak"] is not None),
                      ("same-bits", lambda c: not c["spec"] and c["M"] == total)):
        with pytest.raises(AssertionError, match=r"^\[%s\]" % tag):
            S.check_direct(twisted(when), 96, 32, tag=None)
    with pytest.raises(AssertionError, match=r"^\[same-bits\]"):
        S.check_impulse(twisted(lambda c: not c["spec"]), "imp-32x8-exact", "one", tag=None)
    with pytest.raises(AssertionError, match=r"^\[split-bits\]"):
        S.check_rounding(twisted(lambda c: c["chunk"].shape[1] == 1), "round-32x8-B3", "tiny", tag=None, cache={})


def test_zz_log_the_twin_figures():
    for (tag, tier), (ratio, name) in sorted(S.FIGS.items()):
        if tag in (TAG, "chain"):
            S.H.log_line("stft_stream %-8s WORST %-32s %.4f  (%s)" % (tag, tier, ratio, name))
    S.H.log_line("stft_stream %-8s impulse tier: %d of %d non-zero elements off float32(reference)" % (TAG, COUNT[0], COUNT[1]))
