"""The oracle of the streaming-kernel tests (csrc/stream.hip: ``lstm_state_step`` and ``wn_stream_kernel`` behind
``ops.lstm_stack_state`` and ``ops.wavenet_stream``): float64 references, the case lists, the kernels' form choices restated
in Python, float32 CPU stand-ins with seeded mutants, and ONE assertion function per family, ``check_lstm_state`` and
``check_enc_stream``.  An assertion function takes the implementation under test as a callable: tests/test_stream_kernels_gpu.py
passes the HIP path, tests/test_stream_kernels_cpu.py the float32 stand-ins (the bounds must be within reach of a correct
float32 evaluation) and the mutants (every assertion must be able to fail).  Every comparison is element-wise and goes through
``head_ref.report`` with family "s-lstm" or "s-enc": error, bound and ratio reach the parity log.  There is no aggregate or
relative-L2 alternative anywhere.

The references.  ``lstm_stack_state`` is the packed LSTM stack of ``oracle.head.lstm_layer`` with (h0, c0) in and (h_n, c_n)
out: a row's state stops at its length, padded output steps are zero, length 0 passes the state through.  The streaming
encoder's reference is NOT a streaming algorithm: per row and per utterance (a reset starts a new one) everything the row was
fed is concatenated, ``oracle.wavenet.encode`` runs the valid Conv1d stack on it in float64, then bottleneck, ReLU and the mean
over frames of k columns from column RF - 1 on.  It also keeps every layer's float64 input columns, which is what the rings of
the state block are compared with.

The schedules.  A case's schedule is a list of calls, each a per-row sample count or a reset, driven through
``avvad.stream.FrameClock.advance`` so that the skips are the clock's own.  Every schedule but S5's has: a call in which every
row is still warming up (out_frames = 0, no output buffer), a call with n_b = 1, a call with n_b = 0 for one row beside busy
rows, a call of more than 256 columns, a row whose warm-up is split over three calls, rows with fewer frames than out_frames,
and a row that is reset mid-way and starts a second utterance while the others run on; the rows' column counts differ, so
their rings are at different phases.  The padding behind a row's n_b samples is 1e4: a read beyond n_valid shows.
S5 (filter_width = 1; ``wavenet_autoencoder`` builds with it) has no warm-up, and FrameClock then admits only multiples of k:
neither the split warm-up nor n_b = 1 exists for it; its rows get different cuts, a zero and a reset.

The state block.  After the last call every row's block is held to the documented layout: words 0/1 the 64-bit count of
columns consumed since the row's last reset, exactly; words 2/3 and the alignment padding 0; the causal ring bit for bit the
sample at the newest column congruent to the slot modulo fw - 1; every residual ring slot the float64 layer input at the
newest column congruent to the slot modulo the ring length.  The issue asks for the rings of every row that has consumed
RF - 1 + max h_i columns; here every SLOT is checked whose newest column lies behind its own layer's warm-up (column >=
(fw - 1)(1 + d_0 + .. + d_{i-1})), which contains those rows and also reaches S8, whose four frames per row end before 2559
columns.  The 64-bit count is read and written by the kernel but not exercised beyond 32 bits: a crafted header near 2^32
columns would need the ring rotation restated here.

The mutants of the encoder stand-in are schedule bugs and must be caught by the frame comparisons alone (the stand-in has no
ring state and returns None for it).  ``reset_keeps_history``: the stand-in owns, like the kernel's header, the row's column
count and takes its warm-up from it (asserted equal to the clock's skip when unmutated); the mutant's reset leaves count and
history alone, so the second utterance's first RF - 1 columns, computed on the first utterance's tail, are pooled.  (A reset
that kept the history but still dropped the clock's skip would be no bug at all: the dropped columns are exactly the ones that
see the history.)

Bounds: measured, not chosen.  The project's bounds are the ceilings -- 1e-4 absolute for y and h_n, 1e-4 + 1e-5 |ref| for c_n,
``encoder_ref.OUT_BOUND`` x max(1, max|ref|) for frames and ring slots.  Per family the bound is the smaller of the ceiling and
8 x the worst error of the float32 stand-in against the float64 reference over the case list, rounded up to one significant
digit (8 = a second valid float32 summation order, MFMA's chain, within 1 x of exact, and 4 x head-room: encoder_ref's
factor).  Measured by tests/test_stream_kernels_cpu.py, one thread:

  s-lstm  y, h_n: worst |d| 2.3e-7 (R1; R2 .. R7: 5.9e-8 .. 1.3e-7)           -> LSTM_BOUND   = 2e-6 absolute
          c_n:    worst |d| / (1 + 0.1 |ref|) 5.1e-7 (R1; R2 .. R7: 1.2e-7 .. 4.2e-7) -> LSTM_C_BOUND = 5e-6 + 5e-7 |ref|
  s-enc   frames: worst |d| / max(1, max|ref|) 1.9e-7 (S3; S8: 1.6e-7, the others 3.9e-8 .. 1.3e-7)
                                                                               -> ENC_BOUND    = 2e-6 x max(1, max|ref|)

all far inside the ceilings.  The CPU test asserts that the stand-ins stay at or below 1/8 of these.  The measurement is
against the reference, never against the HIP path."""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

import encoder_ref as E
import head_ref as H
from oracle import wavenet as ow

FAM_LSTM = "s-lstm"
FAM_ENC = "s-enc"
HEADROOM = 8.0
LSTM_CEILING, LSTM_C_CEILING, ENC_CEILING = 1e-4, 1e-4, E.OUT_BOUND      # c_n: atol, with rtol = atol / 10
LSTM_BOUND = 2e-6             # y, h_n: absolute
LSTM_C_BOUND = 5e-6           # c_n: LSTM_C_BOUND + 0.1 LSTM_C_BOUND |ref|
ENC_BOUND = 2e-6              # frames and ring slots: x max(1, max|ref|)
PAD = 1e4                     # what lies behind a row's n_b samples in a chunk


def cdiv(a, b):
    return -(-a // b)


def round_up_1(v):
    """v rounded up to one significant digit"""
    e = int(np.floor(np.log10(v)))
    m = int(np.ceil(v / 10.0 ** e - 1e-9))
    return float("%de%d" % (m, e))


def derived_bound(worst, ceiling):
    return min(ceiling, round_up_1(HEADROOM * worst))


# ------------------------------------------------------------------------------------------ the form choices, restated
# csrc/stream.hip: state_form and the grid of avvad_lstm_layer_fwd_state; the MFMA condition, stream_state_floats,
# stream_lds_bytes and the NC search of avvad_wavenet_stream_fwd.
WS_HDR, WS_NT, WS_NC_MFMA, WS_LDS_MAX = 4, 512, 256, 150 * 1024


def lstm_state_form(B, H, aligned=True):
    """(NG, VEC, grid): NG groups of 16 batch rows per workgroup, 16-byte loads, (hidden quads, column runs)"""
    NG = 1 if B <= 16 else (2 if B <= 32 else 4)
    return NG, bool(H % 4 == 0 and aligned), (cdiv(H, 4), cdiv(B, 16 * NG))


def _geom(cfg):
    return (cfg["filter_width"], cfg["quantization_channel"], cfg["en_residual_channel"], cfg["en_dilation_channel"],
            cfg["en_bottleneck_width"])


def stream_state_floats(cfg):
    fw, qc, R, _, _ = _geom(cfg)
    return cdiv(WS_HDR + (fw - 1) * (qc + R * sum(cfg["dilations"])), 4) * 4


def stream_lds_bytes(cfg, mf, NC):
    _, _, R, D, Bn = _geom(cfg)
    return (R * NC + (96 * 33 if mf else D * NC) + 32 * (NC + 1) + WS_NT + Bn) * 4


def enc_stream_form(cfg):
    """("MFMA", 256) or ("DIRECT", NC): NC the longest pass whose LDS fits, a multiple of 32 where possible"""
    fw, _, R, D, _ = _geom(cfg)
    if R == 32 and D == 32 and fw == 2:
        return "MFMA", WS_NC_MFMA
    NC = WS_NC_MFMA
    while NC > 32 and stream_lds_bytes(cfg, False, NC) > WS_LDS_MAX:
        NC -= 32
    while NC > 1 and stream_lds_bytes(cfg, False, NC) > WS_LDS_MAX:
        NC -= 1
    assert stream_lds_bytes(cfg, False, NC) <= WS_LDS_MAX
    return "DIRECT", NC


def ring_lengths(cfg):
    """h_i = (fw - 1) d_i"""
    return [(cfg["filter_width"] - 1) * d for d in cfg["dilations"]]


def layer_offsets(cfg):
    """the first column (sample index since the reset) at which layer i's input exists: (fw - 1)(1 + d_0 + .. + d_{i-1})"""
    hc, off, s = cfg["filter_width"] - 1, [], 1
    for d in cfg["dilations"]:
        off.append(hc * s)
        s += d
    return off


# ------------------------------------------------------------------------------------------ LSTM with state
LSTM_PARAMS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
LSTM_MUTANTS = ("state_runs_on", "c0_ignored_in_layer_1", "len0_row_zeroed")


def lstm_stack_state(x, lengths, sd, layers, h0, c0, mutant=None):
    """x (B,T,In), h0 / c0 (layers,B,H) -> (y (B,T,H), h_n, c_n); plain torch, dtype-generic, torch's gate order i,f,g,o.
    ``mutant``: ``state_runs_on`` (the state keeps updating past a row's length, so the padded output steps stop being
    zero), ``c0_ignored_in_layer_1`` (layer 1 starts from c = 0), ``len0_row_zeroed`` (a row of length 0 gets a zero state
    back instead of its own)."""
    assert mutant is None or mutant in LSTM_MUTANTS, mutant
    B, T, _ = x.shape
    lengths = torch.as_tensor(lengths)
    y, hn, cn = x, [], []
    for l in range(layers):
        w_ih, w_hh, b_ih, b_hh = (sd["%s_l%d" % (p, l)] for p in LSTM_PARAMS)
        h, c = h0[l], c0[l]
        if mutant == "c0_ignored_in_layer_1" and l == 1:
            c = torch.zeros_like(c)
        outs = []
        for t in range(T):
            gates = y[:, t] @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
            i, f, g, o = gates.chunk(4, dim=1)
            i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
            c_new = f * c + i * g
            h_new = o * torch.tanh(c_new)
            live = (t < lengths)[:, None]
            if mutant == "state_runs_on":
                live = torch.ones_like(live)
            c = torch.where(live, c_new, c)
            h = torch.where(live, h_new, h)
            outs.append(torch.where(live, h_new, torch.zeros_like(h_new)))
        if mutant == "len0_row_zeroed":
            dead = (lengths == 0)[:, None]
            h, c = torch.where(dead, torch.zeros_like(h), h), torch.where(dead, torch.zeros_like(c), c)
        y = torch.stack(outs, dim=1)
        hn.append(h)
        cn.append(c)
    return y, torch.stack(hn), torch.stack(cn)


# In = 40 and one layer unless stated; ``form`` = (NG, VEC, grid) is what lstm_state_form gives (held to it by
# tests/test_stream_kernels_cpu.py).  ``splits``: the chunkings of the T steps, each compared with the float64
# whole-sequence reference.  ``in_place``: the new state is written into the tensors the old one is read from.
LSTM_STATE_CASES = {
    # the audio model's own row
    "R1": dict(B=1, H=1024, In=513, T=3, layers=2, form=(1, True, (256, 1))),
    # two groups of 16 columns, the second with 15 clamped
    "R2": dict(B=17, H=64, T=4, layers=2, form=(2, True, (16, 1))),
    # H % 16 = 8: the last K chunk is half filled under 16-byte loads
    "R3": dict(B=33, H=72, T=3, form=(4, True, (18, 1))),
    # H % 4 != 0: scalar loads, a workgroup with surplus units, two column runs
    "R4": dict(B=70, H=50, In=9, T=3, layers=2, form=(4, False, (13, 2))),
    # T = 1 in place: the staged copy; T = 2 in place: the ping-pong buffers
    "R5-T1": dict(B=16, H=64, T=1, in_place=True, form=(1, True, (16, 1))),
    "R5-T2": dict(B=16, H=64, T=2, in_place=True, form=(1, True, (16, 1))),
    # chunk invariance
    "R6": dict(B=5, H=20, In=7, T=6, layers=2, splits=([1] * 6, [6], [2, 1, 3]), form=(1, True, (5, 1))),
    # the null-hprev form: the recurrent product of the first step is skipped
    "R7": dict(B=17, H=64, T=4, layers=2, state=False, same_as="R2", form=(2, True, (16, 1))),
}


@functools.lru_cache(maxsize=None)
def lstm_state_inputs(name):
    """weights as ``head_ref.lstm_inputs`` draws them (nn.LSTM's own initialisation), x normal, h0 uniform in (-1, 1),
    c0 normal x 2, lengths in [0, T] with lens[0] = T and, where B > 1, lens[-1] = 0"""
    c = LSTM_STATE_CASES[name]
    B, Hd, T, layers, In = c["B"], c["H"], c["T"], c.get("layers", 1), c.get("In", 40)
    rng = np.random.default_rng(sum(map(ord, c.get("same_as", name))) * 104729 + B + Hd + T)
    lens = [int(n) for n in rng.integers(0, T + 1, B)]
    lens[0] = T
    if B > 1:
        lens[-1] = 0
    k = 1.0 / np.sqrt(Hd)
    sd = {}
    for l in range(layers):
        i = In if l == 0 else Hd
        for p, shape in (("weight_ih", (4 * Hd, i)), ("weight_hh", (4 * Hd, Hd)), ("bias_ih", (4 * Hd,)), ("bias_hh", (4 * Hd,))):
            sd["%s_l%d" % (p, l)] = torch.from_numpy(rng.uniform(-k, k, shape).astype(np.float32))
    x = torch.from_numpy(rng.standard_normal((B, T, In)).astype(np.float32))
    h0 = torch.from_numpy(rng.uniform(-1, 1, (layers, B, Hd)).astype(np.float32))
    c0 = torch.from_numpy((2 * rng.standard_normal((layers, B, Hd))).astype(np.float32))
    has_state = c.get("state", True)
    return types.SimpleNamespace(name=name, B=B, H=Hd, T=T, In=In, layers=layers, lens=lens, sd=sd, x=x,
                                 h0=h0 if has_state else None, c0=c0 if has_state else None,
                                 splits=tuple(tuple(s) for s in c.get("splits", ([T],))), in_place=bool(c.get("in_place")))


@functools.lru_cache(maxsize=None)
def lstm_state_reference(name):
    """float64, the whole sequence in one piece: (y, h_n, c_n)"""
    inp = lstm_state_inputs(name)
    z = torch.zeros(inp.layers, inp.B, inp.H, dtype=torch.float64)
    return lstm_stack_state(inp.x.double(), inp.lens, {k: v.double() for k, v in inp.sd.items()}, inp.layers,
                            z if inp.h0 is None else inp.h0.double(), z if inp.c0 is None else inp.c0.double())


def torch_lstm(inp):
    m = torch.nn.LSTM(inp.In, inp.H, inp.layers)
    m.load_state_dict(inp.sd)
    return m.eval()


def _one_thread(fn):
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad():
            return fn()
    finally:
        torch.set_num_threads(n)


def lstm_state_fp32(inp, x, lens, state, in_place=False, mutant=None):
    """The float32 CPU stand-in: ``torch.nn.LSTM`` row by row on one thread (a packed batch cannot hold a length 0); with
    ``mutant``, ``lstm_stack_state`` in float32.  Same signature and result as the GPU callable: dict(y, h, c, h_in, c_in),
    h_in / c_in what the caller's state tensors hold after the call (None without a state)."""
    B, T, _ = x.shape
    zeros = torch.zeros(inp.layers, B, inp.H)
    h0, c0 = (zeros, zeros) if state is None else state
    keep = None if state is None else (h0.clone(), c0.clone())

    def run():
        if mutant is not None:
            return lstm_stack_state(x, lens, inp.sd, inp.layers, h0, c0, mutant)
        m = torch_lstm(inp)
        y, hn, cn = torch.zeros(B, T, inp.H), h0.clone(), c0.clone()
        for b, n in enumerate(lens):
            if n:
                o, (h, c) = m(x[b:b + 1, :n].transpose(0, 1).contiguous(), (h0[:, b:b + 1].contiguous(), c0[:, b:b + 1].contiguous()))
                y[b, :n], hn[:, b], cn[:, b] = o[:, 0], h[:, 0], c[:, 0]
        return y, hn, cn
    y, hn, cn = _one_thread(run)
    h_in, c_in = (None, None) if keep is None else ((hn, cn) if in_place else keep)
    return dict(y=y, h=hn, c=cn, h_in=h_in, c_in=c_in)


def _cpu(t):
    return None if t is None else t.detach().cpu()


def check_lstm_state(impl, name, tag="gpu"):
    """``impl(inp, x, lens, state, in_place)`` -> dict(y, h, c, h_in, c_in): the next steps ``x`` (B,n,In) with per-row
    counts ``lens`` from ``state`` = (h, c) (layers,B,H) or None; h_in / c_in: what the tensors it read the state from
    hold after the call.  For every chunking of the case, y, h_n and c_n element-wise against the float64 whole-sequence
    reference, and as bit-exact facts: a row with no step in a call keeps its (h, c) and gets a zero output; the caller's
    state is untouched unless the call is in place (then it IS the new state); state=None equals an all-zero state.
    -> the worst error / bound of (y and h_n, c_n)."""
    inp = lstm_state_inputs(name)
    ref_y, ref_h, ref_c = lstm_state_reference(name)
    worst_yh = worst_c = 0.0
    for split in inp.splits:
        assert sum(split) == inp.T
        t = "%s%s " % (name, "" if len(inp.splits) == 1 else " chunks %s" % (list(split),))
        state = None if inp.h0 is None else (inp.h0.clone(), inp.c0.clone())
        ys, t0 = [], 0
        for n in split:
            ln = [min(max(l - t0, 0), n) for l in inp.lens]
            x = inp.x[:, t0:t0 + n].contiguous()
            before = None if state is None else (state[0].clone(), state[1].clone())
            r = {k: _cpu(v) for k, v in impl(inp, x, ln, state, inp.in_place).items()}
            assert tuple(r["y"].shape) == (inp.B, n, inp.H) and tuple(r["h"].shape) == tuple(r["c"].shape) == (inp.layers, inp.B, inp.H)
            if before is not None:
                now = (r["h"], r["c"]) if inp.in_place else before
                assert torch.equal(r["h_in"], now[0]) and torch.equal(r["c_in"], now[1]), \
                    t + ("in place: the state tensors do not hold the new state" if inp.in_place else "the caller's state was written")
            for b, nb in enumerate(ln):
                if nb == 0:
                    hb, cb = (0 * r["h"][:, b], 0 * r["c"][:, b]) if before is None else (before[0][:, b], before[1][:, b])
                    assert torch.equal(r["h"][:, b], hb) and torch.equal(r["c"][:, b], cb), t + "row %d has no step and lost its state" % b
                if nb < n:
                    assert float(r["y"][b, nb:].abs().max()) == 0.0, t + "row %d: padded output steps are not zero" % b
            if t0 == 0 and split == inp.splits[0]:
                zeros = (torch.zeros(inp.layers, inp.B, inp.H), torch.zeros(inp.layers, inp.B, inp.H))
                ra, rb = impl(inp, x, ln, None, False), impl(inp, x, ln, zeros, False)
                for k in ("y", "h", "c"):
                    assert torch.equal(_cpu(ra[k]), _cpu(rb[k])), t + "state=None and a zero state differ in " + k
            state = (r["h"].clone(), r["c"].clone())
            ys.append(r["y"])
            t0 += n
        worst_yh = max(worst_yh, H.report(FAM_LSTM, t + "y", torch.cat(ys, 1), ref_y, LSTM_BOUND, tag=tag),
                       H.report(FAM_LSTM, t + "h_n", state[0], ref_h, LSTM_BOUND, tag=tag))
        worst_c = max(worst_c, H.report(FAM_LSTM, t + "c_n", state[1], ref_c, LSTM_C_BOUND, 0.1 * LSTM_C_BOUND, tag=tag))
    return worst_yh, worst_c


# ------------------------------------------------------------------------------------------ streaming encoder: cases
# R = D = 32, fw = 2, qc = 1, biases on unless stated.  ``form`` is what enc_stream_form gives (held to it by
# tests/test_stream_kernels_cpu.py, with the other claims of each line).
ENC_CASES = {
    # a ring longer than a pass (h = 300 > NC), passes shorter than that ring (np < h: the ring is partly rewritten),
    # Bn % 32 != 0 (two bn0 rounds, the second with clamped rows), a frame over two passes
    "S1": dict(dil=[1, 2, 300, 3], Bn=40, k=100, B=3, seed=31, form=("MFMA", 256)),
    # a frame carried through pacc across three passes
    "S2": dict(dil=[1, 2], Bn=32, k=600, B=2, seed=32, form=("MFMA", 256)),
    # one column per frame
    "S3": dict(dil=[4], Bn=32, k=1, B=2, seed=33, form=("MFMA", 256)),
    # the direct form with hc = 2; n: null bias pointers
    "S4": dict(R=16, D=24, fw=3, qc=2, dil=[1, 2, 5], Bn=40, k=9, B=3, seed=34, form=("DIRECT", 256)),
    "S4n": dict(R=16, D=24, fw=3, qc=2, dil=[1, 2, 5], Bn=40, k=9, B=3, bias=False, seed=35, form=("DIRECT", 256)),
    # hc = 0: the state is the header alone, no warm-up
    "S5": dict(R=16, D=24, fw=1, qc=2, dil=[1, 2, 5], Bn=40, k=4, B=3, seed=36, form=("DIRECT", 256),
               schedule=([4, 260, 0], [8, 4, 4], [0, 12, 264], ("reset", 1), [4, 4, 0], [260, 8, 4])),
    # the LDS cap cuts NC to a multiple of 32 below 256
    "S6": dict(R=64, D=64, dil=[1, 3], Bn=32, k=50, B=2, seed=37, form=("DIRECT", 224)),
    # NC < 32: the second loop of the search
    "S7": dict(R=600, D=600, dil=[1, 3], Bn=8, k=20, B=2, seed=38, form=("DIRECT", 30)),
    # the W0 stack at full depth, four frames per row, rings of 512 at different phases
    "S8": dict(dil=E.W0_DIL, Bn=256, k=64, B=2, seed=39, form=("MFMA", 256),
               schedule=([2, 1000], [2045 + 64, 1], [0, 1046 + 128], [64, 0], ("reset", 1), [128, 2047 + 64], [0, 64])),
}


def enc_config(name):
    c = ENC_CASES[name]
    return dict(filter_width=c.get("fw", 2), quantization_channel=c.get("qc", 1), dilations=list(c["dil"]),
                en_residual_channel=c.get("R", 32), en_dilation_channel=c.get("D", 32), en_bottleneck_width=c["Bn"],
                en_pool_kernel_size=1, use_bias=c.get("bias", True))


def generic_schedule(W, k, B):
    """The schedule of a case with a warm-up of W >= 3 samples (see the module docstring for what it contains).  Row 0
    warms up in two calls and then runs steadily, row 1 warms up in three (the second of one sample) and is reset before
    call 5, row 2 starts one call late."""
    assert W >= 3 and B in (2, 3)
    big = cdiv(257, k) * k
    a = (W - 1) // 2
    rows = [[2, W - 2 + k, big, 0, 2 * k, k],
            [a, 1, W - a - 1 + 2 * k, k, W + k, big],
            [0, W, big, k, 0, 2 * k]][:B]
    calls = [[r[i] for r in rows] for i in range(6)]
    return tuple(calls[:4] + [("reset", 1)] + calls[4:])


@functools.lru_cache(maxsize=None)
def enc_inputs(name):
    """float32, drawn as ``encoder_ref.inputs`` draws: parameters from ``oracle.wavenet.init_params``, samples uniform in
    (-1, 1), seeded per case.  ``calls``: the schedule after FrameClock -- ("reset", rows) or a namespace(n, skip, frames,
    out_frames, chunk (B, qc, max(1, max n)) with PAD behind each row's samples)."""
    from avvad.stream import FrameClock
    c, cfg = ENC_CASES[name], enc_config(name)
    B, k, qc = c["B"], c["k"], cfg["quantization_channel"]
    rf = ow.receptive_field(cfg["filter_width"], cfg["dilations"])
    gen = torch.Generator().manual_seed(c["seed"])
    params = ow.init_params(cfg, generator=gen)
    schedule = c.get("schedule") or generic_schedule(rf - 1, k, B)
    clock = FrameClock(B, rf, k)
    calls = []
    for item in schedule:
        if item[0] == "reset":
            rows = [int(r) for r in item[1:]]
            clock.reset(rows)
            calls.append(("reset", rows))
            continue
        n = [int(v) for v in item]
        frames, skip = clock.advance(n)
        chunk = torch.full((B, qc, max(1, max(n))), PAD)
        for b, nb in enumerate(n):
            chunk[b, :, :nb] = torch.rand(qc, nb, generator=gen) * 2 - 1
        calls.append(types.SimpleNamespace(n=n, skip=skip, frames=frames, out_frames=max(frames), chunk=chunk))
    return types.SimpleNamespace(name=name, cfg=cfg, params=params, B=B, k=k, rf=rf, Bn=c["Bn"], calls=tuple(calls))


def run_calls(inp):
    return [c for c in inp.calls if not isinstance(c, tuple)]


# ------------------------------------------------------------------------------------------ streaming encoder: reference
def _tail(params, s):
    return F.relu(F.conv1d(s, params["bottleneck_layer.weight"], params.get("bottleneck_layer.bias")))


def encode_utterance(params, x, cfg, k):
    """x (qc, N), everything a row was fed in one utterance, through ``oracle.wavenet.encode``'s stack in x's dtype ->
    (frames (nf, Bn): the means over k columns from column RF - 1 on, inter: the input columns (R, N - offset_i) of
    every residual layer)"""
    dil, Bn = cfg["dilations"], cfg["en_bottleneck_width"]
    assert x.shape[1] >= ow.receptive_field(cfg["filter_width"], dil), "an utterance of the schedules reaches its first frame"
    _, inter = ow.encode(params, x[None], cfg, return_intermediates=True)
    a = _tail(params, inter[-1])[0]                           # (Bn, N - (RF - 1))
    nf = a.shape[1] // k
    frames = a[:, :nf * k].reshape(Bn, nf, k).mean(2).t()
    return frames, [s[0] for s in inter[:len(dil)]]


@functools.lru_cache(maxsize=None)
def enc_reference(name):
    """float64, per row: the utterances [namespace(x (qc,N) float32 as fed, frames (nf,Bn), inter)], and per run call and row
    where its frames lie: where[call][b] = (utterance, first frame, frames)"""
    inp = enc_inputs(name)
    p64 = {k: v.double() for k, v in inp.params.items()}
    fed = [[[]] for _ in range(inp.B)]
    emitted = [[0] for _ in range(inp.B)]
    where = []
    for c in inp.calls:
        if isinstance(c, tuple):
            for b in c[1]:
                fed[b].append([])
                emitted[b].append(0)
            continue
        w = []
        for b in range(inp.B):
            fed[b][-1].append(c.chunk[b, :, :c.n[b]])
            w.append((len(fed[b]) - 1, emitted[b][-1], c.frames[b]))
            emitted[b][-1] += c.frames[b]
        where.append(w)
    utts = []
    for b in range(inp.B):
        row = []
        for u, parts in enumerate(fed[b]):
            x = torch.cat(parts, 1)
            with torch.no_grad():
                frames, inter = encode_utterance(p64, x.double(), inp.cfg, inp.k)
            assert frames.shape[0] == emitted[b][u], (name, b, u, frames.shape, emitted[b][u])
            row.append(types.SimpleNamespace(x=x, frames=frames, inter=inter))
        utts.append(row)
    return types.SimpleNamespace(utts=utts, where=where)


# ------------------------------------------------------------------------------------------ streaming encoder: stand-in
ENC_MUTANTS = ("history_off_by_one", "reset_keeps_history", "mean_over_valid_only")
PASS = 256                    # columns per recompute of the stand-in


def enc_stream_fp32(inp, mutant=None):
    """The float32 CPU stand-in, a recompute streamer on one thread: per row the last RF - 1 samples (zeros at the start of
    an utterance) and the count of samples since the reset; a call is walked in passes of PASS columns, each the oracle's
    stack on history + pass, the row's remaining warm-up columns are dropped and the rest averaged in frames of k, a
    frame that straddles two passes carried as a partial sum.  It obeys the schedule: cuts, resets, n = 0, and the skip
    it derives from its own count is the clock's.  ``mutant``: ``history_off_by_one`` (what is kept at the end of a call is
    shifted one sample into the past), ``reset_keeps_history`` (a reset leaves history and count alone, so no warm-up
    column of the next utterance is dropped), ``mean_over_valid_only`` (a frame that straddles a pass boundary is divided
    by the columns of its last part).  -> dict(outs: per run call (B, out_frames, Bn), state: None, states: None)"""
    assert mutant is None or mutant in ENC_MUTANTS, mutant
    cfg, k, W, Bn = inp.cfg, inp.k, inp.rf - 1, inp.Bn
    qc = cfg["quantization_channel"]
    hist = [torch.zeros(qc, W) for _ in range(inp.B)]
    seen = [0] * inp.B

    def run():
        outs = []
        for c in inp.calls:
            if isinstance(c, tuple):
                for b in c[1]:
                    if mutant != "reset_keeps_history":
                        hist[b], seen[b] = torch.zeros(qc, W), 0
                continue
            out = torch.zeros(inp.B, c.out_frames, Bn)
            for b, n in enumerate(c.n):
                if n == 0:
                    continue
                skip = max(0, W - seen[b])
                assert mutant is not None or skip == c.skip[b], (inp.name, b, skip, c.skip[b])
                acc, f = torch.zeros(Bn), 0
                for p0 in range(0, n, PASS):
                    npass = min(PASS, n - p0)
                    buf = torch.cat([hist[b], c.chunk[b, :, p0:p0 + npass]], 1)
                    a = _tail(inp.params, ow.encode(inp.params, buf[None], cfg, return_intermediates=True)[1][-1])[0]
                    assert a.shape[1] == npass
                    last = p0 + npass == n
                    hist[b] = buf[:, buf.shape[1] - W - 1:buf.shape[1] - 1] if (mutant == "history_off_by_one" and last) \
                        else buf[:, buf.shape[1] - W:]
                    j = max(skip - p0, 0)
                    while j < npass and f < c.out_frames:
                        fe = skip + (f + 1) * k - p0              # pass-local end of frame f
                        e = min(fe, npass)
                        part = a[:, j:e].sum(1)
                        if fe <= npass:
                            straddles = skip + f * k - p0 < 0
                            div = float(e - j) if (mutant == "mean_over_valid_only" and straddles) else float(k)
                            out[b, f] = (acc + part) / div
                            acc, f = torch.zeros(Bn), f + 1
                        else:
                            acc = acc + part
                        j = e
                seen[b] += n
            outs.append(out)
        return outs
    return dict(outs=_one_thread(run), state=None, states=None)


# ------------------------------------------------------------------------------------------ streaming encoder: assertion
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def check_state_block(name, block, b, tag="gpu"):
    """row b's state block after the last call against the documented layout (see the module docstring)"""
    inp, ref = enc_inputs(name), enc_reference(name)
    cfg = inp.cfg
    fw, qc, R, _, _ = _geom(cfg)
    hc = fw - 1
    utt = ref.utts[b][-1]
    N = utt.x.shape[1]
    block = block.detach().cpu()
    assert block.numel() == stream_state_floats(cfg)
    hdr = _bits(block[:WS_HDR]).tolist()
    t = "%s row %d " % (name, b)
    assert hdr == [N, 0, 0, 0], t + "header %s, %d columns consumed since the reset" % (hdr, N)
    pos = WS_HDR
    if hc:
        ring = block[pos:pos + qc * hc].reshape(qc, hc)
        for s in range(hc):
            col = N - 1 - ((N - 1 - s) % hc) if N > s else -1        # the newest column congruent to s
            want = utt.x[:, col] if col >= 0 else torch.zeros(qc)
            assert torch.equal(_bits(ring[:, s]), _bits(want)), t + "causal ring slot %d is not sample %d" % (s, col)
    pos += qc * hc
    worst = 0.0
    for i, (h, off) in enumerate(zip(ring_lengths(cfg), layer_offsets(cfg))):
        ring = block[pos:pos + R * h].reshape(R, h)
        pos += R * h
        assert N >= h
        slots = [s for s in range(h) if N - 1 - ((N - 1 - s) % h) >= off]
        if not slots:
            continue
        cols = torch.tensor([N - 1 - ((N - 1 - s) % h) - off for s in slots])
        want = utt.inter[i][:, cols]
        worst = max(worst, H.report(FAM_ENC, t + "ring %d (h = %d, %d of %d slots)" % (i, h, len(slots), h), ring[:, slots], want,
                                    ENC_BOUND * max(1.0, float(want.abs().max())), tag=tag))
    if pos < block.numel():
        assert float(block[pos:].abs().max()) == 0.0, t + "the padding behind the rings was written"
    return worst


def check_enc_stream(impl, name, tag="gpu"):
    """``impl(inp)`` -> dict(outs, state, states): outs the (B, out_frames, Bn) of every run call in order, state the
    (B, floats) state tensor after the last call and states its copy after every run call -- both None for an
    implementation without ring state.  Every emitted frame of every row and utterance against the float64 reference;
    frames a row does not fill exactly 0; with a state: a row with n_b = 0 keeps its block bit for bit, and every block
    after the last call against the layout (``check_state_block``).  -> the worst error / bound."""
    inp, ref = enc_inputs(name), enc_reference(name)
    got = impl(inp)
    calls = run_calls(inp)
    assert len(got["outs"]) == len(calls)
    worst = 0.0
    for ci, (c, out, w) in enumerate(zip(calls, got["outs"], ref.where)):
        out = out.detach().cpu()
        assert tuple(out.shape) == (inp.B, c.out_frames, inp.Bn), (name, ci, out.shape)
        for b, (u, f0, nf) in enumerate(w):
            t = "%s call %d row %d " % (name, ci, b)
            if nf < c.out_frames:
                assert float(out[b, nf:].abs().max()) == 0.0, t + "frames the row does not fill are not 0"
            if nf:
                want = ref.utts[b][u].frames[f0:f0 + nf]
                worst = max(worst, H.report(FAM_ENC, t + "utterance %d frames %d..%d (n = %d, skip = %d)" % (u, f0, f0 + nf - 1, c.n[b], c.skip[b]),
                                            out[b, :nf], want, ENC_BOUND * max(1.0, float(want.abs().max())), tag=tag))
    if got["state"] is None:
        return worst
    states = [s.detach().cpu() for s in got["states"]]
    assert len(states) == len(calls) and torch.equal(_bits(states[-1]), _bits(got["state"]))
    prev, si = torch.zeros_like(states[0]), 0
    for c in inp.calls:
        if isinstance(c, tuple):
            prev = prev.clone()
            prev[c[1]] = 0
            continue
        for b, n in enumerate(c.n):
            if n == 0:
                assert torch.equal(_bits(states[si][b]), _bits(prev[b])), "%s: row %d has n = 0 and its state block changed" % (name, b)
        prev, si = states[si], si + 1
    for b in range(inp.B):
        worst = max(worst, check_state_block(name, got["state"][b], b, tag=tag))
    return worst
