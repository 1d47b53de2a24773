"""The streaming kernels on the GPU (csrc/stream.hip) -- ``ops.lstm_stack_state`` and ``ops.wavenet_stream`` with
``ops.wavenet_stream_state``, fed directly with no session in between -- against the float64 references of
tests/stream_ref.py: every LSTM case (y, h_n, c_n element-wise, and the bit-exact facts about rows without a step, the
caller's state and state=None) and every encoder case (every emitted frame of every row and utterance, exact zeros where a
row fills no frame, an untouched state block at n_b = 0, and after the last call every row's state block against the
documented layout: count header, causal ring, residual rings).  The cases, bounds and assertion functions are stream_ref's;
tests/test_stream_kernels_cpu.py runs the same cases with float32 CPU stand-ins in the place of the HIP path and holds every
case to the kernel form it claims.  Then three bit-exact properties: a column of ``lstm_state_step`` does not depend on NG,
VEC or the other columns; an encoder row does not depend on its neighbours; two runs give the same bits."""
import pytest
import torch

import head_ref as H
import stream_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAG = "gpu"


# ------------------------------------------------------------------------------------------ the HIP path as a callable
def _lstm_module(inp):
    m = S.torch_lstm(inp).to(DEV)
    if S.LSTM_STATE_CASES[inp.name]["form"][1]:
        aligned = all(getattr(m, "weight_hh_l%d" % l).data_ptr() % 16 == 0 for l in range(inp.layers))
        assert aligned, "weight_hh off a 16-byte boundary: the case would not reach the form it claims"
    return m


def lstm_gpu(inp, x, lens, state, in_place=False):
    from avvad import ops
    m = _lstm_module(inp)
    st = None if state is None else tuple(t.to(DEV).contiguous() for t in state)
    assert st is None or all(t.data_ptr() % 16 == 0 for t in st)
    y, (h, c) = ops.lstm_stack_state(x.to(DEV), lens, m, state=st, out=st if in_place else None)
    torch.cuda.synchronize()
    if in_place:
        assert h is st[0] and c is st[1]
    return dict(y=y, h=h, c=c, h_in=None if st is None else st[0], c_in=None if st is None else st[1])


def _encoder(inp):
    from packages.models.wavenet_autoencoder import wavenet_autoencoder
    m = wavenet_autoencoder(**inp.cfg)
    m.load_state_dict(inp.params)
    return m.to(DEV).eval()


def enc_gpu(inp, perturb=None):
    """the case's schedule through ops.wavenet_stream; a reset zeroes the rows' state blocks.  ``perturb``: added to the
    samples of rows 1.. in every call and, after the first call, to their state blocks behind the header."""
    from avvad import ops
    enc = _encoder(inp)
    assert enc.receptive_field == inp.rf
    state = ops.wavenet_stream_state(enc, inp.B, DEV)
    assert tuple(state.shape) == (inp.B, S.stream_state_floats(inp.cfg)) and float(state.abs().max()) == 0.0
    outs, states = [], []
    for c in inp.calls:
        if isinstance(c, tuple):
            state.index_fill_(0, torch.tensor(c[1], device=DEV), 0.0)
            continue
        chunk = c.chunk.to(DEV)
        if perturb is not None:
            chunk[1:] += perturb
        outs.append(ops.wavenet_stream(chunk, c.n, c.skip, enc, state, inp.k, c.out_frames))
        if perturb is not None and not states:
            state[1:, S.WS_HDR:] += perturb
        states.append(state.clone())
    torch.cuda.synchronize()
    return dict(outs=outs, state=state, states=states)


# ------------------------------------------------------------------------------------------ against the float64 references
@pytest.mark.parametrize("name", list(S.LSTM_STATE_CASES))
def test_lstm_state(name):
    """what each case reaches: ``stream_ref.LSTM_STATE_CASES``"""
    S.check_lstm_state(lstm_gpu, name, tag=TAG)


@pytest.mark.parametrize("name", list(S.ENC_CASES))
def test_encoder_stream(name):
    """what each case reaches: ``stream_ref.ENC_CASES``"""
    S.check_enc_stream(enc_gpu, name, tag=TAG)


# ------------------------------------------------------------------------------------------ bit-exact properties
def _off_boundary(*shape):
    """a contiguous tensor one float off a 16-byte boundary"""
    n = 1
    for s in shape:
        n *= s
    t = torch.empty(n + 4, dtype=torch.float32, device=DEV)
    first = 1 if t.data_ptr() % 16 == 0 else (16 - t.data_ptr() % 16) // 4 + 1
    v = t[first:first + n].view(*shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def test_lstm_column_does_not_depend_on_ng_vec_or_the_other_columns():
    """With x = 0 the input projection is exactly b_ih in any summation order, so a step's result depends on the recurrent
    product alone.  One layer, H = 64, T = 1, random state: B = 65 (NG = 4, two column runs), its rows 0 .. 15 alone (NG = 1),
    and B = 65 with state and out one float off a 16-byte boundary (VEC off: the scalar-load form with H % 4 == 0) agree
    bit for bit in y, h_n and c_n on the rows they share; the first run is also held to the float64 reference."""
    from avvad import ops
    B, Hd, In = 65, 64, 40
    assert S.lstm_state_form(B, Hd) == (4, True, (16, 2)) and S.lstm_state_form(16, Hd)[0] == 1
    gen = torch.Generator().manual_seed(65)
    k = 1.0 / Hd ** 0.5
    sd = {"weight_ih_l0": (torch.rand(4 * Hd, In, generator=gen) * 2 - 1) * k, "weight_hh_l0": (torch.rand(4 * Hd, Hd, generator=gen) * 2 - 1) * k,
          "bias_ih_l0": (torch.rand(4 * Hd, generator=gen) * 2 - 1) * k, "bias_hh_l0": (torch.rand(4 * Hd, generator=gen) * 2 - 1) * k}
    h0 = torch.rand(1, B, Hd, generator=gen) * 2 - 1
    c0 = torch.randn(1, B, Hd, generator=gen) * 2
    m = torch.nn.LSTM(In, Hd, 1)
    m.load_state_dict(sd)
    m = m.to(DEV)
    assert m.weight_hh_l0.data_ptr() % 16 == 0
    x = torch.zeros(B, 1, In, device=DEV)
    hd, cd = h0.to(DEV), c0.to(DEV)
    ya, (ha, ca) = ops.lstm_stack_state(x, [1] * B, m, state=(hd, cd))
    yb, (hb, cb) = ops.lstm_stack_state(x[:16].contiguous(), [1] * 16, m, state=(hd[:, :16].contiguous(), cd[:, :16].contiguous()))
    hm, cm, ho, co = (_off_boundary(1, B, Hd) for _ in range(4))
    hm.copy_(hd)
    cm.copy_(cd)
    yc, (hc, cc) = ops.lstm_stack_state(x, [1] * B, m, state=(hm, cm), out=(ho, co))
    torch.cuda.synchronize()
    assert hc is ho and cc is co and torch.equal(hm, hd) and torch.equal(cm, cd)
    for what, a, b, c in (("y", ya, yb, yc), ("h_n", ha, hb, hc), ("c_n", ca, cb, cc)):
        rows = a[:16] if what == "y" else a[:, :16]
        assert torch.equal(rows, b), what + ": NG = 4 and NG = 1 differ on the shared rows"
        assert torch.equal(a, c), what + ": 16-byte and scalar loads differ"
    ry, rh, rc = S.lstm_stack_state(torch.zeros(B, 1, In, dtype=torch.float64), [1] * B, {k_: v.double() for k_, v in sd.items()}, 1,
                                    h0.double(), c0.double())
    H.report(S.FAM_LSTM, "B65 H64 x=0 y", ya, ry, S.LSTM_BOUND, tag=TAG)
    H.report(S.FAM_LSTM, "B65 H64 x=0 h_n", ha, rh, S.LSTM_BOUND, tag=TAG)
    H.report(S.FAM_LSTM, "B65 H64 x=0 c_n", ca, rc, S.LSTM_C_BOUND, 0.1 * S.LSTM_C_BOUND, tag=TAG)
    H.log_line("head %-5s %-8s B65 H64 x=0: NG = 4 / NG = 1 / scalar loads bit-identical in y, h_n, c_n" % (TAG, S.FAM_LSTM))


def _same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(S._bits(x), S._bits(y)) for x, y in zip(a, b))


def test_encoder_rows_are_isolated_and_runs_are_bit_identical():
    """S1 three times: twice as it is (same bits in every output and every state snapshot), once with the samples and
    state blocks of rows 1 and 2 perturbed (row 0's frames and state block bit-identical, the others' not)"""
    inp = S.enc_inputs("S1")
    a, b, p = enc_gpu(inp), enc_gpu(inp), enc_gpu(inp, perturb=0.25)
    assert _same_bits(a["outs"], b["outs"]) and _same_bits(a["states"], b["states"])
    assert _same_bits([o[0] for o in a["outs"]], [o[0] for o in p["outs"]]), "row 0's frames changed when only rows 1 and 2 did"
    assert _same_bits([s[0] for s in a["states"]], [s[0] for s in p["states"]]), "row 0's state block changed when only rows 1 and 2 did"
    assert not _same_bits([o[1:] for o in a["outs"]], [o[1:] for o in p["outs"]])
    H.log_line("head %-5s %-8s S1 twice: outputs and states bit-identical; row 0 bit-identical under changes to rows 1-2" % (TAG, S.FAM_ENC))


def test_lstm_runs_are_bit_identical():
    inp = S.lstm_state_inputs("R2")
    runs = [lstm_gpu(inp, inp.x, inp.lens, (inp.h0, inp.c0)) for _ in range(2)]
    for k in ("y", "h", "c"):
        assert torch.equal(S._bits(runs[0][k]), S._bits(runs[1][k])), k
    H.log_line("head %-5s %-8s R2 twice: y, h_n, c_n bit-identical" % (TAG, S.FAM_LSTM))


def test_zz_log_worst_ratios():
    H.log_worst(TAG)
