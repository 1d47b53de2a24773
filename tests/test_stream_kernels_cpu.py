"""CPU tests of the streaming-kernel oracle (tests/stream_ref.py): every case of tests/test_stream_kernels_gpu.py with the
float32 CPU stand-ins in the place of the HIP path (the measured bounds are within reach of a correct float32 evaluation at
1/8, and the harness works), seeded mutants that the assertion functions must reject on a named case, the case lists against
the restated form choices of csrc/stream.hip, the float64 streaming-encoder reference against ``oracle.wavenet.encode``, the
float64 LSTM against ``oracle.head.lstm_stack``, and the restated state size against the library's."""
import ctypes as C

import pytest
import torch

import head_ref as H
import stream_ref as S
from oracle import head as oh
from oracle import wavenet as ow

TAG = "cpu32"
EIGHTH = 1.0 / S.HEADROOM + 1e-6


# ------------------------------------------------------------------------------------------ the references
def test_lstm_reference_is_the_oracle_from_a_zero_state():
    """``lstm_stack_state`` from h0 = c0 = 0 against ``oracle.head.lstm_stack`` in float64, and its h_n against the output at
    each row's last valid step"""
    inp = S.lstm_state_inputs("R6")
    sd = {k: v.double() for k, v in inp.sd.items()}
    z = torch.zeros(inp.layers, inp.B, inp.H, dtype=torch.float64)
    y, hn, cn = S.lstm_stack_state(inp.x.double(), inp.lens, sd, inp.layers, z, z)
    assert float((y - oh.lstm_stack(inp.x.double(), inp.lens, sd, "", inp.layers)).abs().max()) <= 1e-14
    for b, n in enumerate(inp.lens):
        assert torch.equal(hn[-1, b], y[b, n - 1] if n else z[0, b])
        assert float(y[b, n:].abs().max() if n < inp.T else 0.0) == 0.0


def test_lstm_reference_is_chunk_invariant_and_passes_length_0_through():
    inp = S.lstm_state_inputs("R6")
    sd = {k: v.double() for k, v in inp.sd.items()}
    whole = S.lstm_state_reference("R6")
    h, c, ys, t0 = inp.h0.double(), inp.c0.double(), [], 0
    for n in (2, 1, 3):
        ln = [min(max(l - t0, 0), n) for l in inp.lens]
        y, h, c = S.lstm_stack_state(inp.x[:, t0:t0 + n].double(), ln, sd, inp.layers, h, c)
        ys.append(y)
        t0 += n
    for got, ref in ((torch.cat(ys, 1), whole[0]), (h, whole[1]), (c, whole[2])):
        assert float((got - ref).abs().max()) <= 1e-14
    assert inp.lens[-1] == 0 and torch.equal(whole[1][:, -1], inp.h0[:, -1].double()) and torch.equal(whole[2][:, -1], inp.c0[:, -1].double())


@pytest.mark.parametrize("name,P", [("S1", 3), ("S4", 7), ("S4n", 2), ("S5", 5), ("S8", 2)])
def test_streaming_reference_at_one_call_is_the_oracle(name, P):
    """L = RF - 1 + P k samples: the adaptive pool has uniform windows of k, and ``encode_utterance`` in float64 equals
    ``oracle.wavenet.encode`` with en_pool_kernel_size = P; its layer inputs are the oracle's intermediates"""
    inp = S.enc_inputs(name)
    p64 = {k: v.double() for k, v in inp.params.items()}
    gen = torch.Generator().manual_seed(P)
    x = torch.rand(inp.cfg["quantization_channel"], inp.rf - 1 + P * inp.k, generator=gen, dtype=torch.float64) * 2 - 1
    with torch.no_grad():
        frames, inter = S.encode_utterance(p64, x, inp.cfg, inp.k)
        ref, ref_inter = ow.encode(p64, x[None], dict(inp.cfg, en_pool_kernel_size=P), return_intermediates=True)
    assert tuple(frames.shape) == (P, inp.Bn)
    assert float((frames.t() - ref[0]).abs().max()) <= 1e-14 * max(1.0, float(ref.abs().max()))
    off = S.layer_offsets(inp.cfg)
    for i, s in enumerate(inter):
        assert torch.equal(s, ref_inter[i][0]) and s.shape[1] == x.shape[1] - off[i]


def test_streaming_reference_splits_utterances_at_a_reset():
    """S1: row 1 has two utterances, the others one; every emitted frame is accounted for"""
    inp, ref = S.enc_inputs("S1"), S.enc_reference("S1")
    assert [len(u) for u in ref.utts] == [1, 2, 1]
    for b in range(inp.B):
        fed = sum(c.n[b] for c in S.run_calls(inp))
        assert sum(u.x.shape[1] for u in ref.utts[b]) == fed
        assert sum(u.frames.shape[0] for u in ref.utts[b]) == sum(c.frames[b] for c in S.run_calls(inp))
    assert all(u.frames.dtype == torch.float64 for row in ref.utts for u in row)


# ------------------------------------------------------------------------------------------ what the case lists reach
def test_case_lists_reach_what_they_claim():
    # ---- LSTM: (NG, VEC, grid) of every case; between them NG = 1, 2, 4 and both load forms
    for name, c in S.LSTM_STATE_CASES.items():
        inp = S.lstm_state_inputs(name)
        assert S.lstm_state_form(inp.B, inp.H) == c["form"], name
        assert inp.lens[0] == inp.T and (inp.B == 1 or inp.lens[-1] == 0), name
        assert (inp.h0 is None) == (name == "R7")
        if inp.h0 is not None:
            assert float(inp.h0.abs().min()) > 0 and float(inp.h0.abs().max()) < 1 and float(inp.c0.abs().max()) > 2
    forms = {name: c["form"] for name, c in S.LSTM_STATE_CASES.items()}
    assert {f[0] for f in forms.values()} == {1, 2, 4} and {f[1] for f in forms.values()} == {True, False}
    L = S.LSTM_STATE_CASES
    assert (L["R1"]["B"], L["R1"]["H"], L["R1"]["In"], L["R1"]["layers"]) == (1, 1024, 513, 2)
    assert forms["R2"][0] == 2 and 32 - L["R2"]["B"] == 15                       # 15 clamped columns
    assert forms["R3"][0] == 4 and L["R3"]["H"] % 16 == 8 and L["R3"]["H"] % 4 == 0
    assert L["R4"]["H"] % 4 != 0 and forms["R4"] == (4, False, (13, 2)) and 13 * 4 > L["R4"]["H"]     # surplus units, two runs
    assert S.lstm_state_form(70, 52) == (4, True, (13, 2)) and S.lstm_state_form(70, 52, aligned=False)[1] is False
    assert L["R5-T1"]["in_place"] and L["R5-T2"]["in_place"] and (L["R5-T1"]["T"], L["R5-T2"]["T"]) == (1, 2)
    assert L["R6"]["splits"] == ([1] * 6, [6], [2, 1, 3])
    r2, r7 = S.lstm_state_inputs("R2"), S.lstm_state_inputs("R7")
    assert all(torch.equal(r2.sd[k], r7.sd[k]) for k in r2.sd) and torch.equal(r2.x, r7.x) and r2.lens == r7.lens
    # the bit-exact independence test of the GPU file: B = 65 (NG = 4, two runs), its first 16 rows (NG = 1), VEC off
    assert S.lstm_state_form(65, 64) == (4, True, (16, 2)) and S.lstm_state_form(16, 64) == (1, True, (16, 1))
    assert S.lstm_state_form(65, 64, aligned=False) == (4, False, (16, 2))

    # ---- encoder: the form and NC of every case; between them MFMA and the three kinds of NC of the direct form
    E = S.ENC_CASES
    for name, c in E.items():
        cfg = S.enc_config(name)
        assert S.enc_stream_form(cfg) == c["form"], name
        assert S.stream_lds_bytes(cfg, c["form"][0] == "MFMA", c["form"][1]) <= S.WS_LDS_MAX
    kinds = {("MFMA" if f == "MFMA" else "DIRECT-256" if nc == 256 else "DIRECT-32s" if nc % 32 == 0 else "DIRECT-odd")
             for f, nc in (c["form"] for c in E.values())}
    assert kinds == {"MFMA", "DIRECT-256", "DIRECT-32s", "DIRECT-odd"}
    cfg6, cfg7 = S.enc_config("S6"), S.enc_config("S7")
    assert E["S6"]["form"] == ("DIRECT", 224) and S.stream_lds_bytes(cfg6, False, 256) > S.WS_LDS_MAX
    assert E["S7"]["form"] == ("DIRECT", 30) and S.stream_lds_bytes(cfg7, False, 32) > S.WS_LDS_MAX \
        and S.stream_lds_bytes(cfg7, False, 31) > S.WS_LDS_MAX
    NC = {name: c["form"][1] for name, c in E.items()}
    # S1: a ring longer than a pass, a pass shorter than that ring, clamped bottleneck rows, a frame over two passes
    assert max(S.ring_lengths(S.enc_config("S1"))) == 300 > NC["S1"] and E["S1"]["Bn"] % 32 == 8
    assert any(0 < n < 300 for c in S.run_calls(S.enc_inputs("S1")) for n in c.n)
    assert any(n - s > NC["S1"] and (NC["S1"] - s) % E["S1"]["k"] for c in S.run_calls(S.enc_inputs("S1")) for n, s in zip(c.n, c.skip))
    # S2: a frame over three passes; S3: one column per frame; S4n: no bias; S5: no history at all
    assert E["S2"]["k"] > 2 * NC["S2"] and E["S3"]["k"] == 1
    assert S.enc_config("S4")["use_bias"] and not S.enc_config("S4n")["use_bias"] and "en_causal_layer.bias" not in S.enc_inputs("S4n").params
    assert S.enc_config("S4")["filter_width"] - 1 == 2 and S.enc_config("S5")["filter_width"] == 1
    assert S.stream_state_floats(S.enc_config("S5")) == S.WS_HDR and S.enc_inputs("S5").rf == 1
    # S7: frames of k < NC columns that straddle passes of 30; S8: W0, four frames per row, rings of 512 at different phases
    assert E["S7"]["k"] % NC["S7"] != 0
    assert E["S8"]["dil"] == ow.W0["dilations"] and S.enc_inputs("S8").rf == 2048
    s8 = S.enc_inputs("S8")
    assert [sum(c.frames[b] for c in S.run_calls(s8)) for b in range(2)] == [4, 4]
    counts = [u[-1].x.shape[1] for u in S.enc_reference("S8").utts]
    assert counts[0] % 512 != counts[1] % 512

    # ---- the schedules: what every case's calls contain
    for name in E:
        inp, ref = S.enc_inputs(name), S.enc_reference(name)
        calls = S.run_calls(inp)
        ns = [n for c in calls for n in c.n]
        assert any(n > 256 for n in ns), name
        assert any(0 in c.n and max(c.n) > 0 for c in calls), name
        assert any(len(u) == 2 for u in ref.utts) and any(len(u) == 1 for u in ref.utts), name           # a reset row beside others
        assert any(0 < c.frames[b] < c.out_frames for c in calls for b in range(inp.B)), name              # zero fill
        assert len({tuple(c.n[b] for c in calls) for b in range(inp.B)}) == inp.B, name                     # rows differ
        if name == "S5":
            assert all(s == 0 for c in calls for s in c.skip)
            continue
        assert 1 in ns, name
        assert any(c.out_frames == 0 and max(c.n) > 0 for c in calls), name
        warm = [[c.n[b] for c in calls if 0 < c.skip[b] and c.n[b] > 0][:3] for b in range(inp.B)]
        assert any(len(w) == 3 and sum(w[:2]) < inp.rf - 1 <= sum(w) for w in warm), (name, warm)           # warm-up in three calls
        assert any(0 < s < n for c in calls for n, s in zip(c.n, c.skip)), name                             # warm-up ends inside a call


def test_restated_state_size_is_the_librarys():
    from avvad import _lib as L
    h = L.lib()
    for name in S.ENC_CASES:
        cfg = S.enc_config(name)
        dil = (C.c_int * len(cfg["dilations"]))(*cfg["dilations"])
        d = L.WavenetDesc(S.ENC_CASES[name]["B"], 1, cfg["quantization_channel"], cfg["en_residual_channel"], cfg["en_dilation_channel"],
                          cfg["en_bottleneck_width"], cfg["filter_width"], 1, len(cfg["dilations"]), dil, int(cfg["use_bias"]), 0, 0)
        assert h.avvad_wavenet_stream_state_bytes(C.byref(d)) == 4 * S.stream_state_floats(cfg), name
    assert S.stream_state_floats(ow.W0) == 4 + 1 + 32 * 2046 + 3


# ------------------------------------------------------------------------------------------ the stand-ins under the checks
def _worst_of_this_case(family, run):
    before = H.WORST.pop((TAG, family), None)
    result = run()
    now = H.WORST[(TAG, family)]
    if before is not None and before[0] > now[0]:
        H.WORST[(TAG, family)] = before
    return result


@pytest.mark.parametrize("name", list(S.LSTM_STATE_CASES))
def test_float32_lstm_passes_at_an_eighth_of_the_bounds(name):
    yh, c = _worst_of_this_case(S.FAM_LSTM, lambda: S.check_lstm_state(S.lstm_state_fp32, name, tag=TAG))
    print("%s: y, h_n %.3e of %.0e; c_n %.3e of %.0e (x (1 + 0.1 |ref|))" % (name, yh * S.LSTM_BOUND, S.LSTM_BOUND, c * S.LSTM_C_BOUND, S.LSTM_C_BOUND))
    assert yh <= EIGHTH and c <= EIGHTH, (yh, c)


@pytest.mark.parametrize("name", list(S.ENC_CASES))
def test_float32_streamer_passes_at_an_eighth_of_the_bound(name):
    r = _worst_of_this_case(S.FAM_ENC, lambda: S.check_enc_stream(S.enc_stream_fp32, name, tag=TAG))
    print("%s: %.3e of %.0e (x max(1, max|ref|))" % (name, r * S.ENC_BOUND, S.ENC_BOUND))
    assert r <= EIGHTH, r


def test_bounds_are_below_the_projects_ceilings():
    assert S.LSTM_BOUND <= S.LSTM_CEILING == 1e-4 and S.LSTM_C_BOUND <= S.LSTM_C_CEILING == 1e-4 and S.ENC_BOUND <= S.ENC_CEILING == 2e-5
    assert S.round_up_1(1.86e-6) == 2e-6 and S.round_up_1(2e-6) == 2e-6 and S.round_up_1(4.06e-6) == 5e-6
    assert S.derived_bound(1e-3, 1e-4) == 1e-4 and S.derived_bound(2.32e-7, 1e-4) == S.LSTM_BOUND


def test_lstm_stand_in_mutated_without_a_mutant_is_the_restatement():
    """the float32 restatement the mutants are built on passes the check itself: a mutant fails because of its mutation"""
    for name in ("R2", "R4", "R6"):
        S.check_lstm_state(lambda inp, x, ln, st, ip: _restated(inp, x, ln, st, ip, None), name, tag=None)


def _restated(inp, x, ln, st, in_place, mutant):
    z = torch.zeros(inp.layers, inp.B, inp.H)
    h0, c0 = (z, z) if st is None else st
    keep = None if st is None else (h0.clone(), c0.clone())
    with torch.no_grad():
        y, h, c = S.lstm_stack_state(x, ln, inp.sd, inp.layers, h0, c0, mutant)
    h_in, c_in = (None, None) if keep is None else ((h, c) if in_place else keep)
    return dict(y=y, h=h, c=c, h_in=h_in, c_in=c_in)


# ------------------------------------------------------------------------------------------ mutants
@pytest.mark.parametrize("mutant,name,what", [
    ("state_runs_on", "R2", "padded output steps are not zero"), ("state_runs_on", "R6", "R6 chunks"),
    ("c0_ignored_in_layer_1", "R2", "R2 "), ("c0_ignored_in_layer_1", "R1", "R1 "), ("c0_ignored_in_layer_1", "R4", "R4 "),
    ("len0_row_zeroed", "R3", "lost its state"), ("len0_row_zeroed", "R5-T1", "lost its state"), ("len0_row_zeroed", "R6", "lost its state")])
def test_lstm_mutant_is_rejected(mutant, name, what):
    assert name in S.LSTM_STATE_CASES
    S.check_lstm_state(S.lstm_state_fp32, name, tag=None)                         # the unmutated stand-in passes there
    with pytest.raises(AssertionError, match=what) as e:
        S.check_lstm_state(lambda inp, x, ln, st, ip: S.lstm_state_fp32(inp, x, ln, st, ip, mutant=mutant), name, tag=None)
    print(str(e.value).splitlines()[0])


def test_lstm_check_sees_a_written_caller_state_and_a_wrong_zero_state():
    def writes_state(inp, x, ln, st, ip):
        r = S.lstm_state_fp32(inp, x, ln, st, ip)
        if st is not None:
            r["h_in"] = r["h"]
        return r
    with pytest.raises(AssertionError, match="caller's state was written"):
        S.check_lstm_state(writes_state, "R2", tag=None)

    def none_is_not_zero(inp, x, ln, st, ip):
        r = S.lstm_state_fp32(inp, x, ln, st, ip)
        if st is None:
            r["c"] = r["c"] + 1e-7
        return r
    with pytest.raises(AssertionError, match="state=None and a zero state differ"):
        S.check_lstm_state(none_is_not_zero, "R3", tag=None)


@pytest.mark.parametrize("mutant,name", [
    ("history_off_by_one", "S1"), ("history_off_by_one", "S4"), ("history_off_by_one", "S7"), ("history_off_by_one", "S8"),
    ("reset_keeps_history", "S1"), ("reset_keeps_history", "S2"), ("reset_keeps_history", "S8"),
    ("mean_over_valid_only", "S1"), ("mean_over_valid_only", "S2"), ("mean_over_valid_only", "S6"), ("mean_over_valid_only", "S7")])
def test_streamer_mutant_is_rejected(mutant, name):
    """by a FRAME comparison (or a frame that should be zero): the stand-in has no ring state"""
    assert name in S.ENC_CASES
    S.check_enc_stream(S.enc_stream_fp32, name, tag=None)                         # the unmutated stand-in passes there
    with pytest.raises(AssertionError, match="frames") as e:
        S.check_enc_stream(lambda inp: S.enc_stream_fp32(inp, mutant=mutant), name, tag=None)
    print(str(e.value).splitlines()[0])


@pytest.mark.parametrize("name,b", [("S4", 1), ("S1", 2)])
def test_state_block_check_rejects_wrong_blocks(name, b):
    """``check_state_block`` on a block built from the reference (the stand-in has none): it passes, and a wrong count, a
    non-zero header word, a wrong sample, two swapped ring entries and (S1) a touched padding word are each rejected"""
    cfg, utt = S.enc_inputs(name).cfg, S.enc_reference(name).utts[b][-1]
    N, hc, qc, R = utt.x.shape[1], cfg["filter_width"] - 1, cfg["quantization_channel"], cfg["en_residual_channel"]
    block = torch.zeros(S.stream_state_floats(cfg))
    block[:1] = torch.tensor([N], dtype=torch.int32).view(torch.float32)
    pos = S.WS_HDR
    for col in range(N - hc, N):
        block[pos + torch.arange(qc) * hc + col % hc] = utt.x[:, col]
    pos += qc * hc
    for h, off, s in zip(S.ring_lengths(cfg), S.layer_offsets(cfg), utt.inter):
        for col in range(N - h, N):
            block[pos + torch.arange(R) * h + col % h] = s[:, col - off].float()
        pos += R * h
    assert (pos < block.numel()) == (name == "S1")                               # S1 has padding behind its rings
    assert S.check_state_block(name, block, b, tag=None) <= EIGHTH

    def bad(edit, match):
        blk = block.clone()
        edit(blk)
        with pytest.raises(AssertionError, match=match):
            S.check_state_block(name, blk, b, tag=None)
    bad(lambda t: t[:1].copy_(torch.tensor([N + 1], dtype=torch.int32).view(torch.float32)), "header")
    bad(lambda t: t[2:3].fill_(1.0), "header")
    bad(lambda t: t[S.WS_HDR:S.WS_HDR + 1].add_(1e-7), "causal ring")
    first = S.WS_HDR + qc * hc
    bad(lambda t: t[first:first + 2].copy_(t[first:first + 2].flip(0)), "ring 0")
    if pos < block.numel():
        bad(lambda t: t[-1:].fill_(1e-30), "padding")


def test_zz_log_worst_ratios():
    H.log_worst(TAG)
