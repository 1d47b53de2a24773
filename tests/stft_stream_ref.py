"""The oracle of the streaming STFT front-end tests (csrc/stft_stream.hip and the product it shares with the streaming
inverse, csrc/stream_product.h, behind ``ops.stft_stream`` and ``avvad_stft_stream_fwd`` / ``_fwd_spec``): the stream around
the transform restated from the contract of include/avvad.h, the launch plan RESTATED from ``sprod::plan``, the case list,
the packet policies, a float32 CPU twin in the kernel's summation order with its mutants, and one assertion function per
tier.  The transform itself is tests/stft_ref.py's: its float64 basis, framing, spectrum, frame count, impulse reference and
propagated feature bounds.  An assertion function takes the implementation under test as a callable ``impl(call)`` that
performs ONE kernel-level call (``call``: see ``make_call``) and returns ``dict(out=, spec=, state=)`` as numpy arrays:
tests/test_stft_stream_kernels_gpu.py passes the HIP path, tests/test_stft_stream_ref_cpu.py the twin (every bound must be
within reach of correct float32 arithmetic) and its mutants (every assertion must be able to fail).  A failed assertion
names itself in square brackets, ``[state] ...``: the CPU test asserts which one a mutant trips.

The stream (``ref_call``), from the header and nothing else.  Row b's logical stream is ``state_in[b][:n_pending]`` followed
by ``chunk[b][:n_valid]``; frame t of the call is samples [t hop, t hop + n_fft) of it, zeros past its end -- which only a
row with ``pad_frames`` may reach; out and spec are zero behind a row's frames; the new state is the raw stream from
``n_frames hop`` on, zero behind it, an exact copy, unscaled by the peak; a row with no new sample and no frame keeps its
state bit for bit; counts are clamped by the header's rule (``clamped_counts``; ss_row's cited lines).  ``stream_through``
drives a whole wave through an implementation by a packet policy with the host bookkeeping the header describes (frames
after N samples: max(0, (N - n_fft) / hop + 1); a final row reaches ``stft_ref.n_frames``), checks the state, the zero fill
and the shapes call by call, and hands back each row's frames in order: frame t of a call is frame ``emitted + t`` of the
whole wave, so the values are held to stft_ref's WHOLE-UTTERANCE references.  Behind each row's valid samples the chunk holds
NaN, and so does state_in behind n_pending in the direct-call and clamp cases.

Tiers, one assertion function each.

* IMPULSE (``check_impulse``; every configuration, L = n_fft + 7 hop - 1, + 0, + 1, B = 3, policies one / hop / ragged).
  Impulses +-2^j at least n_fft apart: no summation order rounds anything.  [zero]: exactly 0 where the reference is;
  [spectrum]: |fwd_spec - ref| <= 2^-23 |ref|; [log]: ``log_bound`` with dP = 4 2^-23 P; [silence]: where P = 0,
  float32(log(float64(float32(eps)))) within 2 ulp; [same-bits]: fwd and fwd_spec give the same features (first wave of a
  case).  Impulses sit at sample 0 and L - 1 of every row, left and right of every call boundary of the policy, at k = 0
  and k = n_fft - 1 of every frame that straddles a call's pending tail and chunk, and at k = n_fft - 1 of the pad
  frame's predecessor.  The first sample a pad frame reads as zero is NaN in the chunk, or sample 0 of the next row.
* FRAME MAP AND GRID (the same function): ``rows-130`` (the scan base across three 64-row groups, frames of one pass from
  several rows, more rows than tail-writing workgroups and zero-fill slots), ``many-32x1`` / ``many-32x8-B3`` (gridDim.y
  capped, a second trip of the pass loop), ``ng-edge`` (16, 17, 32, 33 frames), ``fallback-1216`` / ``max-2048`` (21 frames at
  NG = 1).
* ROUNDING (``check_rounding``).  [spectrum]: |got - X| <= (n_fft + 41) 2^-24 S, stft_ref's derived bound (any order of n_fft
  terms with head-room: also eight interleaved chains and seven additions); with a peak that is no power of two the
  reference is the float64 spectrum of float64(float32 x) / float64(float32 peak) and the bound takes one more unit, n_fft +
  42.  [zero] where S = 0.  [aggregate]: relative Frobenius error <= 4 x that of stft_ref's sequential-chain twin.  Each case
  runs under ``one`` and one other policy, which must agree bit for bit ([split-bits]).
* FEATURES (``check_features``): [log] / [standardised] within ``_feature_reference``'s dlog / dstd on the checked elements,
  [aggregate] on the log features, [unchecked] share on the reference alone.  ``feat-32x8-peak3.7`` has a peak that is no
  power of two and a reference of its own; its cap is 0.
* SILENCE (``check_silence``).  * DIRECT CALLS (``check_direct``): d->M as 0, the sum, 1 and 10 x the sum ([hint-bits]),
  d->T = tmax + 3 and d->L = n + 5 ([pitch]), peak NULL against ones ([peak-bits]).  * CLAMPING (``check_clamp``): wrong
  counts, every buffer carved from one arena by the implementation; [clamp]: the outputs are those of the clamped counts,
  [guard]: no guard band changed.  The wrong counts are off by at most 3 samples or 2 frames: unclamped they would reach
  at most 3 floats behind a chunk row, 2 behind a state row, 2 F floats in front of or 2 F behind out and twice that for
  spec -- inside guard bands of 4 n_fft floats.

Measured.  MI355X | float32 twin in the kernel's order | as one sequential chain.  Worst element error / bound, then the
relative Frobenius error of the spectrum (policy ``one``):
  round-1024x256-B3    0.0013 | 0.0007 | 0.0063    2.13e-07 | 1.31e-07 | 5.73e-07
  round-1024x256-tilt  0.0015 | 0.0011 | 0.0086    2.12e-07 | 1.30e-07 | 5.61e-07
  round-512x100-B3     0.0022 | 0.0016 | 0.0091    1.56e-07 | 1.09e-07 | 4.05e-07
  round-96x32-B3       0.0112 | 0.0107 | 0.0398    9.04e-08 | 8.21e-08 | 1.74e-07
  round-32x8-B3        0.0367 | 0.0263 | 0.0585    7.95e-08 | 7.02e-08 | 1.04e-07
  round-1024x1024-B3   0.0009 | 0.0006 | 0.0041    2.09e-07 | 1.30e-07 | 5.61e-07
  round-256x64-B3      0.0041 | 0.0035 | 0.0191    1.19e-07 | 9.56e-08 | 2.86e-07
  round-160x48-B2      0.0068 | 0.0054 | 0.0215    1.08e-07 | 9.35e-08 | 2.22e-07
  round-1184x296-B2    0.0009 | 0.0005 | 0.0036    2.25e-07 | 1.37e-07 | 6.03e-07
  round-1216x304-B2    0.0008 | 0.0005 | 0.0037    2.25e-07 | 1.38e-07 | 6.22e-07
  round-2048x512-B2    0.0005 | 0.0003 | 0.0024    2.91e-07 | 1.66e-07 | 8.06e-07
Feature cases: worst log error / bound, worst standardised error / bound, relative Frobenius error of the log features:
  round-32x8-feat      0.0269 | 0.0239 | 0.0395    0.0604 | 0.0445 | 0.0491    3.33e-07 | 3.16e-07 | 5.16e-07
  round-96x32-feat     0.0109 | 0.0057 | 0.0163    0.0253 | 0.0253 | 0.0260    2.31e-07 | 2.04e-07 | 2.95e-07
  round-512x100-feat   0.0017 | 0.0012 | 0.0043    0.0044 | 0.0027 | 0.0056    2.29e-07 | 1.47e-07 | 3.54e-07
  round-32x8-tilt      0.0836 | 0.0325 | 0.0622    0.1252 | 0.1110 | 0.1129    3.41e-06 | 4.20e-06 | 2.22e-06
  feat-32x8-peak3.7    0.0430 | 0.0203 | 0.0515    0.0631 | 0.0631 | 0.0660    2.09e-06 | 1.25e-06 | 2.82e-06
(the second policy of a case gives the same bits, hence the same figures.  The twin takes an MFMA as its four products
summed, then added to the accumulator; the order inside the instruction is the hardware's own, which is why the twin is no
bit-level model and the MI355X sits between it and the chain.  Eight short chains beat one long one either way.)  The
aggregate's worst share of its allowance on the MI355X is 0.19 of the 4 x (round-32x8-B3).  Impulse tier, MI355X: of the
7 722 074 non-zero elements of all impulse and frame-map cases 0 differ from float32(reference) (worst spectrum error 0.50
ulp, worst log error / bound 0.66); 0 for the twin.  State, zero fill, fwd against fwd_spec, d->M, the pitches, peak NULL and the six clamp variants (guards intact) hold bit
for bit at 96x32 and 1024x256.  A scratch build whose packed basis is evaluated in float32 with an unreduced phase (exact
zeros kept) fails [aggregate] in every rounding case on the MI355X -- 4.30e-05 at round-1024x256-B3, 75 x the chain; 1.16e-06 at
round-32x8-B3, 11 x -- and [spectrum] in the impulse tier; the twin's ``f32_trig_zeros`` mutant shows the same on the CPU.
"""
import functools
import zlib

import numpy as np

import head_ref as H
import stft_ref as R

FAMILY = "stft_stream"
CSRC = R.CSRC
U, ULP = R.U, R.ULP
NW, PAD, LDS_MAX, K_MAX = 8, 4, 150 * 1024, 2048
SS_SLOT_INTS = 5
POLICIES = ("one", "hop", "odd", "ragged", "tiny")

# The lines of the source the restatements rest on, as (file, line, text): test_cited_lines_hold fails when an edit moves one.
CITES = [
    ("stream_product.h", 21, "constexpr int NT = 512;"),
    ("stream_product.h", 23, "constexpr int PAD = 4;"),
    ("stream_product.h", 24, "constexpr size_t LDS_MAX = 150 * 1024;"),
    ("stream_product.h", 25, "constexpr int K_MAX = 2048;"),
    ("stream_product.h", 28, "int operand_index(int K, int kk, int q, int j) { return (K >> 2) * q + 4 * kk + j; }"),
    ("stream_product.h", 58, "const int excl = base + incl - nf;"),
    ("stream_product.h", 65, "base += __shfl(incl, 63, 64);"),
    ("stream_product.h", 88, "for (int kk = wave; kk < KQ; kk += NW) {"),
    ("stream_product.h", 118, "for (int w = 1; w < NW; ++w) v += pf[w * 256];"),
    ("stream_product.h", 130, "const size_t frames = (size_t)16 * NG * (K + PAD) * sizeof(float), parts = (size_t)NG * NP * NW * 64 * sizeof(f32x4);"),
    ("stream_product.h", 133, "return front + align_up((size_t)(tab_ints * 16 * NG + 1) * sizeof(int), 16);"),
    ("stream_product.h", 137, "p.NG = hint > 16 ? 2 : 1;"),
    ("stream_product.h", 139, "if (p.NG == 2 && p.lds > LDS_MAX) p.lds = lds_bytes(K, NP, tab_ints, p.NG = 1, &p.tab);"),
    ("stream_product.h", 140, "const long ny = (hint + 16 * p.NG - 1) / (16 * p.NG);"),
    ("stream_product.h", 141, "p.ny = (int)(ny < 1 ? 1 : (ny > 16 ? 16 : ny));"),
    ("stream_product.h", 142, "if (p.lds > LDS_MAX) p.NG = 0;"),
    ("stft_stream.hip", 17, "constexpr int SS_SLOT_INTS = 5;"),
    ("stft_stream.hip", 57, "r.nv = clamp_count(a.n_valid[b], a.L);"),
    ("stft_stream.hip", 58, "r.np = clamp_count(a.n_pending[b], a.K);"),
    ("stft_stream.hip", 60, "int cap = (Ls >= a.K ? (Ls - a.K) / a.hop + 1 : 0) + (a.pad_frames[b] ? 1 : 0);"),
    ("stft_stream.hip", 61, "if (cap > a.T) cap = a.T;"),
    ("stft_stream.hip", 62, "r.nf = clamp_count(nf, cap);"),
    ("stft_stream.hip", 111, "dst[k] = ss_sample(a, b, r, s0 + k) / pk;"),
    ("stft_stream.hip", 122, "float v = logf(fmaf(re, re, im * im) + a.eps);"),
    ("stft_stream.hip", 123, "if (a.mean) v = (v - a.mean[f]) / (a.stdv[f] + a.norm_eps);"),
    ("stft_stream.hip", 133, "for (int b = blockIdx.y * (sp::NT / 16) + (tid >> 4); b < a.B; b += gridDim.y * (sp::NT / 16)) {"),
    ("stft_stream.hip", 142, "for (int b = blockIdx.y * gridDim.x + nb; b < a.B; b += gridDim.x * gridDim.y) {"),
    ("stft_stream.hip", 146, "if (a.n_valid[b] <= 0 && r.nf == 0) {"),
    ("stft_stream.hip", 172, "const sp::Plan p = sp::plan(K, 2, SS_SLOT_INTS, d->M > 0 ? d->M : (long)d->B * d->T);"),
    ("stft_stream.hip", 176, "const dim3 grid(ss_bin_blocks(K), p.ny);"),
    ("common.h", 103, "int clamp_count(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }"),
]


# ------------------------------------------------------------------------------------------ the plan, restated
def operand_index(K, kk, q, j):           # stream_product.h (line 28)
    return (K >> 2) * q + 4 * kk + j


def lds_bytes(K, NP, tab_ints, NG):
    """stream_product.h lds_bytes (lines 130 .. 133) -> (bytes, float offset of the tables)"""
    frames, parts = 16 * NG * (K + PAD) * 4, NG * NP * NW * 64 * 16
    front = max(frames, parts)
    return front + -(-((tab_ints * 16 * NG + 1) * 4) // 16) * 16, front // 4


def plan(K, NP, tab_ints, hint):
    """sprod::plan (lines 137 .. 142) -> dict(NG, ny, lds); NG = 0: K does not fit"""
    NG = 2 if hint > 16 else 1
    lds = lds_bytes(K, NP, tab_ints, NG)[0]
    if NG == 2 and lds > LDS_MAX:
        NG = 1
        lds = lds_bytes(K, NP, tab_ints, NG)[0]
    ny = min(max(-(-hint // (16 * NG)), 1), 16)
    if lds > LDS_MAX:
        NG = 0
    return dict(NG=NG, ny=ny, lds=lds)


def ss_plan(n_fft, B, T, M=0):
    """the launch of one forward call (stft_stream.hip lines 172, 176) and what its frame counts make of it"""
    p = plan(n_fft, 2, SS_SLOT_INTS, M if M > 0 else B * T)
    p["blocks"] = (n_fft // 2 + 1 + 15) // 16
    return p


def call_reach(n_fft, n_frames, T=None, M=None):
    """what one call with these per-row frame counts reaches"""
    B, total = len(n_frames), int(sum(n_frames))
    p = ss_plan(n_fft, B, max(n_frames) if T is None else T, total if M is None else M)
    FP = 16 * p["NG"]
    passes = -(-total // FP)
    rows_in_pass = max([len(_rows_of_pass(n_frames, m0, FP)) for m0 in range(0, total, FP)] + [0])
    return dict(NG=p["NG"], ny=p["ny"], passes=passes, trips=-(-passes // p["ny"]) if passes else 0,
                idle_waves=max(0, NW - n_fft // 16), uneven=(n_fft // 16) % NW != 0, row_groups=-(-B // 64),
                rows_in_pass=rows_in_pass, rows_over_tail_wgs=B > p["blocks"] * p["ny"], rows_over_fill_slots=B > 32 * p["ny"],
                lds=p["lds"])


def _rows_of_pass(n_frames, m0, FP):
    edges = np.concatenate([[0], np.cumsum(n_frames)])
    return {b for b in range(len(n_frames)) if edges[b] < m0 + FP and edges[b + 1] > m0 and n_frames[b] > 0}


# ------------------------------------------------------------------------------------------ the stream, restated from the header
def _clamp(v, hi):
    return 0 if v < 0 else (hi if v > hi else int(v))


def clamped_counts(call):
    """include/avvad.h: n_valid to [0, L], n_pending to [0, n_fft], n_frames to [0, min(T, complete frames of the n_pending +
    n_valid samples, + 1 with pad_frames)] -> per row (nv, np, nf)"""
    K, hop, Lp, T = call["cfg"]["n_fft"], call["cfg"]["hop"], call["chunk"].shape[1], call["T"]
    rows = []
    for b in range(call["chunk"].shape[0]):
        nv, npd = _clamp(call["n_valid"][b], Lp), _clamp(call["n_pending"][b], K)
        Ls = nv + npd
        cap = ((Ls - K) // hop + 1 if Ls >= K else 0) + (1 if call["pad"][b] else 0)
        rows.append((nv, npd, _clamp(call["n_frames"][b], min(cap, T))))
    return rows


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ref_call(call):
    """what one call must do to each row -> dict(counts, frames: per row (nf, n_fft) float32 RAW samples, state (B, n_fft))"""
    K, hop = call["cfg"]["n_fft"], call["cfg"]["hop"]
    counts = clamped_counts(call)
    frames, state = [], np.zeros((len(counts), K), dtype=np.float32)
    for b, (nv, npd, nf) in enumerate(counts):
        stream = np.concatenate([call["state_in"][b, :npd], call["chunk"][b, :nv]]).astype(np.float32)
        fr = np.zeros((nf, K), dtype=np.float32)
        for t in range(nf):
            seg = stream[t * hop:t * hop + K]
            fr[t, :seg.size] = seg
        frames.append(fr)
        if call["n_valid"][b] <= 0 and nf == 0:
            state[b] = call["state_in"][b]                # idle: bit for bit, whatever lies behind the count
        else:
            tail = stream[nf * hop:][:K]
            state[b, :tail.size] = tail
    return dict(counts=counts, frames=frames, state=state)


def make_call(cfg, chunk, n_valid, n_pending, n_frames, pad, state_in, peak=None, stats=False, spec=True, T=None, M=None,
              plain=False, first=False, final=(), arena=False):
    """One kernel-level call.  chunk (B, L) float32 with L the pitch; the four counts as lists; state_in (B, n_fft); peak (B,)
    or None; stats: standardise with cfg's mean / std; spec: avvad_stft_stream_fwd_spec; T: frame pitch of out (default: the
    largest count), M: the descriptor's hint (default: the sum).  plain: the call is what ``ops.stft_stream`` would build from a
    SampleClock (first: of a fresh one; final: its rows that end), so the HIP path may go through it; arena: carve the
    buffers out of one guarded arena and report the guards."""
    n_frames = [int(v) for v in n_frames]
    return dict(cfg=cfg, chunk=np.ascontiguousarray(chunk, dtype=np.float32), n_valid=[int(v) for v in n_valid],
                n_pending=[int(v) for v in n_pending], n_frames=n_frames, pad=[int(v) for v in pad],
                state_in=np.ascontiguousarray(state_in, dtype=np.float32), peak=None if peak is None else np.asarray(peak, dtype=np.float32),
                stats=bool(stats), spec=bool(spec), T=max(max(n_frames), 0) if T is None else int(T),
                M=max(sum(n_frames), 0) if M is None else int(M), plain=plain, first=first, final=tuple(final), arena=arena)


def _must(tag, ok, msg):
    if not ok:
        raise AssertionError("[%s] %s" % (tag, msg() if callable(msg) else msg))


def _within(tag, name, what, got, ref, bound, mask=None):
    try:
        return R._within(name, what, got, ref, bound, mask)
    except AssertionError as e:
        raise AssertionError("[%s] %s" % (tag, e)) from None


def check_call_shape(name, call, g, r):
    """[shape], [zero-fill], [state] of one call's result against ``ref_call``"""
    B, K = call["state_in"].shape
    T, F = call["T"], K // 2 + 1
    _must("shape", g["out"].shape == (B, T, F) and g["out"].dtype == np.float32, lambda: "%s: out %s" % (name, g["out"].shape))
    if call["spec"]:
        _must("shape", g["spec"].shape == (B, T, F, 2) and g["spec"].dtype == np.float32, lambda: "%s: spec %s" % (name, g["spec"].shape))
    for b, (_, _, nf) in enumerate(r["counts"]):
        rest = [g["out"][b, nf:]] + ([g["spec"][b, nf:]] if call["spec"] else [])
        _must("zero-fill", all(not (bits(x) != 0).any() for x in rest), "%s: row %d is not zero behind its %d frames" % (name, b, nf))
    same = (bits(g["state"]) == bits(r["state"])).all(axis=1)
    _must("state", g["state"].shape == (B, K) and same.all(), lambda: "%s: the new state of row %d is not the stream from "
          "n_frames hop on (first difference at %d)" % (name, int(np.argmin(same)), int(np.argmax(bits(g["state"])[np.argmin(same)]
                                                                                                   != bits(r["state"])[np.argmin(same)]))))


# ------------------------------------------------------------------------------------------ packet policies
def frames_total(L, n_fft, hop):
    return max(R.n_frames(L, n_fft, hop), 0)


def packets(policy, lengths, n_fft, hop, seed=0, explicit=None):
    """-> [(n per row, rows that end)]: every row's samples in calls, the call that takes a row's last sample is its final one
    (a row of no samples never ends: it idles); at most about 300 calls"""
    B = len(lengths)
    left = list(lengths)
    rng = np.random.default_rng(seed)
    calls = []
    while any(left):
        i = len(calls)
        if explicit is not None:
            want = [explicit[i] if i < len(explicit) else 1 << 30] * B
        elif policy == "one" or i >= 300:
            want = [1 << 30] * B
        elif policy == "hop":
            want = [hop] * B
        elif policy == "odd":
            want = [n_fft + 1] * B
        elif policy == "tiny":
            want = [1 if i < n_fft + 2 * hop else 1 << 30] * B
        else:
            assert policy == "ragged", policy
            want = [0 if rng.random() < 0.2 else int(rng.integers(0, 3 * n_fft + 1)) for _ in range(B)]
        n = [min(left[b], want[b]) for b in range(B)]
        fin = [b for b in range(B) if left[b] > 0 and n[b] == left[b]]
        left = [left[b] - n[b] for b in range(B)]
        calls.append((n, fin))
    return calls or [([0] * B, [])]


def stream_through(impl, name, cfg, rows, calls, peak=None, stats=False, spec=True, nan_state=False, plain=True):
    """``rows`` (1-D float32 arrays) through ``impl`` by ``calls``: the host bookkeeping of the header, [shape] / [zero-fill]
    / [state] per call -> dict(out: per row (T_b, F), spec: per row (T_b, F, 2), frames: per row the reference's gather,
    n_frames: per call)"""
    B, K, hop = len(rows), cfg["n_fft"], cfg["hop"]
    total, emitted, ended, pos = [0] * B, [0] * B, [False] * B, [0] * B
    state = np.zeros((B, K), dtype=np.float32)
    outs, specs, gathered, per_call = [[] for _ in rows], [[] for _ in rows], [[] for _ in rows], []
    for ci, (n, fin) in enumerate(calls):
        pend = [max(total[b] - emitted[b] * hop, 0) for b in range(B)]
        nf, pad = [0] * B, [0] * B
        for b in range(B):
            if ended[b]:
                assert n[b] == 0 and b not in fin
                continue
            N = total[b] + n[b]
            e = max(0, (N - K) // hop + 1)
            if b in fin:
                pad[b] = frames_total(N, K, hop) - e
                assert pad[b] in (0, 1)
            nf[b] = e + pad[b] - emitted[b]
            total[b], emitted[b], ended[b] = N, e + pad[b], b in fin
        chunk = np.full((B, max(max(n), 1)), np.nan, dtype=np.float32)
        for b in range(B):
            chunk[b, :n[b]] = rows[b][pos[b]:pos[b] + n[b]]
            pos[b] += n[b]
        state_in = state.copy()
        if nan_state:
            for b in range(B):
                state_in[b, pend[b]:] = np.nan
        call = make_call(cfg, chunk, n, pend, nf, pad, state_in, peak, stats, spec, plain=plain and not nan_state, first=ci == 0, final=fin)
        r = ref_call(call)
        assert [c[2] for c in r["counts"]] == nf, "honest counts are not clamped"
        g = impl(call)
        check_call_shape("%s call %d" % (name, ci), call, g, r)
        state = r["state"]
        per_call.append(nf)
        for b in range(B):
            outs[b].append(g["out"][b, :nf[b]])
            gathered[b].append(r["frames"][b])
            if spec:
                specs[b].append(g["spec"][b, :nf[b]])
    assert pos == [len(x) for x in rows]
    cat = lambda parts: [np.concatenate(p, 0) for p in parts]
    return dict(out=cat(outs), spec=cat(specs) if spec else None, frames=cat(gathered), n_frames=per_call)


# ------------------------------------------------------------------------------------------ the cases
CASES = {}
CONFIGS = ((32, 8), (32, 1), (96, 32), (160, 48), (256, 64), (512, 100), (1024, 256), (1024, 1024), (1184, 296), (1216, 304),
           (2048, 512))


def _case(name, n_fft, hop, lengths, policies, why, signal="impulse", peak=None, base=None, features=False, unchecked_max=None,
          explicit=None, reach=None):
    assert name not in CASES, name
    CASES[name] = dict(name=name, n_fft=n_fft, hop=hop, B=len(lengths), L=max(lengths), lengths=tuple(lengths), pad=True, fs=16e3,
                       eps=1e-8, norm_eps=1e-3, signal=signal, peak=peak, base=base, features=features,
                       unchecked_max=unchecked_max, policies=tuple(policies), explicit=explicit, why=why, reach=reach or {})
    return [(name, p) for p in policies]


def _reuse(base, policies, why, peak=None, reach=None, **kw):
    """a case of stft_ref streamed: its wave, its references"""
    c = R.CASES[base]
    assert c["pad"]
    return _case(base, c["n_fft"], c["hop"], [c["L"]] * c["B"], policies, why, signal=c["signal"], peak=peak, base=base,
                 features=c["features"], unchecked_max=c["unchecked_max"], reach=reach, **kw)


IMPULSE = []
for _n, _h in CONFIGS:
    _idle, _un = max(0, NW - _n // 16), (_n // 16) % NW != 0
    for _d, _w in ((-1, "minus"), (0, "exact"), (1, "plus")):
        IMPULSE += _case("imp-%dx%d-%s" % (_n, _h, _w), _n, _h, [_n + 7 * _h + _d] * 3, ("one", "hop", "ragged"),
                         "n_fft + 7 hop %+d" % _d, reach=dict(idle_waves=_idle, uneven=_un, NG=1 if _n >= 1216 else 2))

_rng = np.random.default_rng(130)
_len130 = [int(v) for v in _rng.integers(0, 401, 130)]
for _b, _v in ((3, 0), (63, 0), (64, 5), (65, 0), (127, 20), (128, 0)):
    _len130[_b] = _v
GRID = _case("rows-130", 32, 8, _len130, ("one", "ragged"), "the scan base across three 64-row groups; rows beyond the tail-writing "
             "workgroups (all) and the zero-fill slots (ragged)", reach=dict(row_groups=3, rows_over_tail_wgs=True, NG=2, idle_waves=6))
GRID += _case("many-32x1", 32, 1, [632], ("one",), "more than 16 x 32 frames: gridDim.y capped, a second trip of the pass loop",
              reach=dict(NG=2, ny=16, passes=19, trips=2))
GRID += _case("many-32x8-B3", 32, 8, [4001] * 3, ("one",), "about 1490 frames", reach=dict(NG=2, ny=16, passes=47, trips=3))
GRID += _case("ng-edge", 1024, 256, [1024 + 97 * 256 - 1], ("edge",), "calls of exactly 16, 17, 32 and 33 frames",
              explicit=[1024 + 15 * 256, 17 * 256, 32 * 256], reach=dict(per_call=[16, 17, 32, 33], NG=2))
GRID += _case("fallback-1216", 1216, 304, [1216 + 20 * 304 - 1], ("one",), "21 frames with NG forced to 1", reach=dict(NG=1, passes=2, ny=2))
GRID += _case("max-2048", 2048, 512, [2048 + 20 * 512 - 1], ("one",), "21 frames at the documented maximum", reach=dict(NG=1, passes=2, ny=2))
RAGGED_POLICY_REACH = dict(name="rows-130", policy="ragged", rows_over_fill_slots=True)

ROUNDING = (_reuse("round-1024x256-B3", ("one", "odd"), "the flagship configuration") +
            _reuse("round-1024x256-tilt", ("one", "hop"), "60 dB tilt") +
            _reuse("round-512x100-B3", ("one", "odd"), "hop does not divide n_fft") +
            _reuse("round-96x32-B3", ("one", "tiny"), "real-modulo phase, 6 groups") +
            _reuse("round-32x8-B3", ("one", "tiny"), "2 groups for 8 waves", peak=0.25) +
            _reuse("round-1024x1024-B3", ("one", "hop"), "hop = n_fft") +
            _reuse("round-256x64-B3", ("one", "hop"), "a peak of 2: the division is exact", peak=2.0))
for _n, _h in ((160, 48), (1184, 296), (1216, 304), (2048, 512)):
    ROUNDING += _case("round-%dx%d-B2" % (_n, _h), _n, _h, [_n + 20 * _h + 3] * 2, ("one", "tiny" if _n == 160 else "ragged"),
                      "white noise", signal="white", reach=dict(NG=1 if _n >= 1216 else 2))
FEATURES = (_reuse("round-32x8-feat", ("one", "ragged"), "white features") +
            _reuse("round-96x32-feat", ("one", "hop"), "white features, the modulo phase") +
            _reuse("round-512x100-feat", ("one", "odd"), "white features on 32 groups") +
            _reuse("round-32x8-tilt", ("one", "odd"), "60 dB tilt") +
            _case("feat-32x8-peak3.7", 32, 8, [400] * 3, ("one", "hop"), "a peak that is no power of two: a reference of its own, one "
                  "more unit in the bound", signal="white", peak=3.7, features=True, unchecked_max=0.0))
SILENCE = (_case("silence-1024x256", 1024, 256, [16000] * 3, ("hop",), "all-zero wave", signal="zero") +
           _case("silence-96x32", 96, 32, [500], ("ragged",), "all-zero wave", signal="zero"))
DIRECT = ((96, 32), (1024, 256))


def cfg_of(c):
    """what an implementation is told about a case; stft_ref's statistics (its std holds a zero: norm_eps alone divides)"""
    return R.cfg_of(dict(c, name=c["base"] or c["name"]))


def case_calls(name, policy):
    c = CASES[name]
    return packets(policy, c["lengths"], c["n_fft"], c["hop"], seed=zlib.crc32((name + policy).encode()), explicit=c["explicit"])


def case_frames_per_call(name, policy):
    """per call, per row: the frame counts the bookkeeping gives"""
    c = CASES[name]
    K, hop, B = c["n_fft"], c["hop"], c["B"]
    total, emitted, out = [0] * B, [0] * B, []
    for n, fin in case_calls(name, policy):
        nf = []
        for b in range(B):
            total[b] += n[b]
            e = (frames_total(total[b], K, hop) if b in fin else max(0, (total[b] - K) // hop + 1)) if (n[b] or b in fin) else emitted[b]
            nf.append(e - emitted[b])
            emitted[b] = e
        out.append(nf)
    return out


def case_reach(name, policy):
    """what the calls of a case under a policy reach together"""
    c = CASES[name]
    per = [call_reach(c["n_fft"], nf) for nf in case_frames_per_call(name, policy)]
    busy = [p for p in per if p["passes"]] or per
    big = max(busy, key=lambda p: p["passes"])
    return dict(NG=big["NG"], ny=big["ny"], passes=big["passes"], trips=big["trips"], idle_waves=big["idle_waves"], uneven=big["uneven"],
                row_groups=big["row_groups"], rows_in_pass=max(p["rows_in_pass"] for p in per),
                rows_over_tail_wgs=any(p["rows_over_tail_wgs"] for p in per), rows_over_fill_slots=any(p["rows_over_fill_slots"] for p in per),
                per_call=[sum(nf) for nf in case_frames_per_call(name, policy)], lds=big["lds"])


# ------------------------------------------------------------------------------------------ signals and references
@functools.lru_cache(maxsize=4)
def signal(name):
    """(B, L) float32, peak-normalised as stft_ref makes it (the stream's RAW samples are this times the case's peak)"""
    c = CASES[name]
    if c["base"]:
        return R.signal(c["base"])
    B, L = c["B"], c["L"]
    if c["signal"] == "zero":
        return np.zeros((B, L), dtype=np.float32)
    assert c["signal"] == "white"
    x = R._peak(np.random.default_rng(zlib.crc32(name.encode())).standard_normal((B, L)))
    x.setflags(write=False)
    return x


def _pow2(v):
    return v is None or float(np.frexp(np.float32(v))[0]) == 0.5


def raw_signal(name):
    """(raw float32 samples the stream carries, peak (B,) or None)"""
    c = CASES[name]
    x = signal(name)
    if c["peak"] is None:
        return x, None
    return (x * np.float32(c["peak"])).astype(np.float32), np.full(c["B"], c["peak"], dtype=np.float32)


@functools.lru_cache(maxsize=2)
def round_reference(name):
    """(X, E, the sequential-chain twin's spectrum, T): stft_ref's own for its cases; for a peak that is no power of two the
    float64 spectrum of float64(float32 x) / float64(float32 peak) with one more unit in the bound"""
    c = CASES[name]
    T = frames_total(c["L"], c["n_fft"], c["hop"])
    if c["base"] and _pow2(c["peak"]):
        return R._round_reference(c["base"]) + (T,)
    raw, peak = raw_signal(name)
    if _pow2(c["peak"]):
        X, S = R.spectrum64(signal(name), c["n_fft"], c["hop"], T)
        units, wave32 = c["n_fft"] + 41, signal(name)
    else:
        A = R.frames_of(raw, c["n_fft"], c["hop"], T).astype(np.float64) / float(np.float32(c["peak"]))
        W = R.basis64(c["n_fft"])
        X, S = A @ W, np.abs(A) @ np.abs(W)
        units, wave32 = c["n_fft"] + 42, (raw / np.float32(c["peak"])).astype(np.float32)
    return X, units * U * S, R.twin_spectrum(wave32, c["n_fft"], c["hop"], T, order="chain"), T


def unchecked_share(name):
    c = CASES[name]
    X, E, _, _ = round_reference(name)
    return float(1.0 - R._feature_reference(c, cfg_of(c), X, E)["checked"].mean())


def required_positions(name, policy):
    """per row: where streaming indexing goes wrong (module docstring)"""
    c = CASES[name]
    K, hop = c["n_fft"], c["hop"]
    need = []
    for b, L in enumerate(c["lengths"]):
        if L == 0:
            need.append([])
            continue
        T = frames_total(L, K, hop)
        mine, N = [0, L - 1], 0
        if T >= 2:
            mine.append((T - 2) * hop + K - 1)            # k = n_fft - 1 of the pad frame's predecessor (or of the last but one)
        for n, _ in case_calls(name, policy):
            if n[b] == 0:
                continue
            if N > 0:
                mine += [N - 1, N]
                e = max(0, (N - K) // hop + 1)             # frames emitted before this call: the tail starts at e hop
                strad = [t for t in range(e, (N + n[b] - K) // hop + 1) if t * hop < N] if N + n[b] >= K else []
                for t in strad:
                    mine += [t * hop, t * hop + K - 1]
            N += n[b]
        need.append([p for p in dict.fromkeys(mine) if 0 <= p < L])
    return need


def impulse_waves(name, policy):
    """-> [(rows, placed per row [(p, a)])], generated like ``stft_ref.impulse_waves``: as many waves as it takes to place every
    required impulse, random ones in what room is left; at least n_fft between two impulses of a row"""
    c = CASES[name]
    K = c["n_fft"]
    rng = np.random.default_rng(zlib.crc32((name + policy).encode()))
    need = required_positions(name, policy)
    waves = []
    while any(need) or not waves:
        rows, placed = [np.zeros(L, dtype=np.float32) for L in c["lengths"]], [[] for _ in c["lengths"]]
        for b, L in enumerate(c["lengths"]):
            left = []
            extra = [int(p) for p in rng.integers(0, L, 3)] if L else []
            for i, p in enumerate(need[b] + extra):
                if all(abs(q - p) >= K for q, _ in placed[b]):
                    a = float(rng.choice([-1.0, 1.0]) * 2.0 ** int(rng.integers(-6, 4)))
                    rows[b][p] = a
                    placed[b].append((p, a))
                elif i < len(need[b]):
                    left.append(p)
            assert not need[b] or len(left) < len(need[b])
            need[b] = left
        waves.append((rows, placed))
    return waves


def impulse_reference(c, placed):
    """per row (T_b, F, 2) float64, exact: ``stft_ref.impulse_reference`` of the row alone"""
    out = []
    for L, pl in zip(c["lengths"], placed):
        if frames_total(L, c["n_fft"], c["hop"]) == 0:
            out.append(np.zeros((0, c["n_fft"] // 2 + 1, 2)))
        else:
            out.append(R.impulse_reference(dict(c, B=1, L=L), [(0, p, a) for p, a in pl])[0])
    return out


# ------------------------------------------------------------------------------------------ the assertion functions
FIGS = {}


def _note(tag, tier, ratio, name):
    if tag is not None and not (ratio <= FIGS.get((tag, tier), (-1.0, ""))[0]):
        FIGS[(tag, tier)] = (ratio, name)


def _log(tag, msg):
    if tag is not None:
        H.log_line("stft_stream %-8s %s" % (tag, msg))


def _exact_tier(name, spec, lg, ref, c, tag):
    """[zero] / [spectrum] / [log] / [silence] of exact spectra: spec (M, F, 2), lg (M, F) or None -> (off, non-zero)"""
    eps = R._eps32(c)
    zero = ref == 0
    _must("zero", not (spec[zero] != 0).any(), lambda: "%s: %d elements are not zero where the spectrum is exactly zero, the first at %s" % (
        name, int((spec[zero] != 0).sum()), tuple(np.argwhere(zero & (spec != 0))[0])))
    _note(tag, "impulse spectrum", _within("spectrum", name, "spectrum", spec, ref, ULP * np.abs(ref)), name)
    if lg is not None:
        P = ref[..., 0] ** 2 + ref[..., 1] ** 2
        dP = 4.0 * ULP * P
        _note(tag, "impulse log", _within("log", name, "log-power", lg, np.log(P + eps), R.log_bound(P, dP, eps), mask=P > 0), name)
        if (P == 0).any():
            _must("silence", np.isfinite(lg).all() and R._ulps(lg[P == 0], R.silence_log(c)).max() <= 2,
                  lambda: "%s: log(0 + eps) is %r, expected %r" % (name, lg[P == 0][0], R.silence_log(c)))
    return int((spec != ref.astype(np.float32)).sum()), int((~zero).sum())


def check_impulse(impl, name, policy, tag="gpu", max_waves=None):
    """-> (elements off float32(reference), non-zero elements)"""
    c, cfg = CASES[name], cfg_of(CASES[name])
    calls = case_calls(name, policy)
    off = total = 0
    for wi, (rows, placed) in enumerate(impulse_waves(name, policy)[:max_waves]):
        ref = np.concatenate(impulse_reference(c, placed), 0)
        res = stream_through(impl, name, cfg, rows, calls)
        o, t = _exact_tier(name, np.concatenate(res["spec"], 0), np.concatenate(res["out"], 0), ref, c, tag)
        off, total = off + o, total + t
        if wi == 0:
            plain = stream_through(impl, name, cfg, rows, calls, spec=False)
            _must("same-bits", all(np.array_equal(bits(a), bits(b)) for a, b in zip(plain["out"], res["out"])),
                  "%s: avvad_stft_stream_fwd and _fwd_spec give different features" % name)
    return off, total                                     # (summed and logged by the tests' last function)


def _run_noise(impl, name, policy, stats=False):
    c = CASES[name]
    raw, peak = raw_signal(name)
    res = stream_through(impl, name, cfg_of(c), [np.array(r) for r in raw], case_calls(name, policy), peak=peak, stats=stats)
    return np.concatenate(res["spec"], 0).reshape(-1, 2 * (c["n_fft"] // 2 + 1)), np.concatenate(res["out"], 0)


def _split_bits(impl, name, policy, key, value, cache):
    """[split-bits]: the policy's result against that of ``one``, bit for bit"""
    if cache is None:
        return
    cache[(name, policy) + key] = value
    if policy != "one":
        one = cache.get((name, "one") + key)
        if one is None:
            one = cache[(name, "one") + key] = _run_noise(impl, name, "one", stats=key == ("std",))
        _must("split-bits", all(a.shape == b.shape and np.array_equal(bits(a), bits(b)) for a, b in zip(one, value)),
              "%s: policy %s and one call give different bits" % (name, policy))


def check_rounding(impl, name, policy, tag="gpu", cache=None):
    """[zero] / [spectrum] / [aggregate] / [split-bits] of a noise case -> dict of figures"""
    X, E, chain, _ = round_reference(name)
    got, lg = _run_noise(impl, name, policy)
    _must("shape", got.shape == X.shape, lambda: "%s: %s frames, expected %s" % (name, got.shape, X.shape))
    _must("zero", not (got[E == 0] != 0).any(), "%s: non-zero where |frames| |basis| is zero" % name)
    worst = _within("spectrum", name, "spectrum", got, X, E)
    fig = dict(worst=worst, fro=R.rel_fro(got, X), fro_twin=R.rel_fro(chain, X))
    _note(tag, "rounding spectrum", worst, name)
    _log(tag, "%-22s %-6s spectrum: worst error / bound %.4f, relative Frobenius error %.3e (sequential float32 twin %.3e)" % (
        name, policy, worst, fig["fro"], fig["fro_twin"]))
    _must("aggregate", fig["fro"] <= R.TWIN_FACTOR * fig["fro_twin"], "%s: relative Frobenius error %.3e, more than %g x the %.3e of a "
          "sequential float32 chain" % (name, fig["fro"], R.TWIN_FACTOR, fig["fro_twin"]))
    _note(tag, "rounding aggregate / (4 x twin)", fig["fro"] / (R.TWIN_FACTOR * fig["fro_twin"]), name)
    _split_bits(impl, name, policy, (), (got, lg), cache)
    return fig


def check_features(impl, name, policy, tag="gpu", cache=None):
    """[unchecked] / [log] / [standardised] / [aggregate] / [split-bits] of a feature case -> dict of figures"""
    c, cfg = CASES[name], cfg_of(CASES[name])
    assert c["features"]
    X, E, chain, T = round_reference(name)
    r = R._feature_reference(c, cfg, X, E)
    share = float(1.0 - r["checked"].mean())
    _must("unchecked", share <= c["unchecked_max"], "%s: %.3f %% of the reference's elements have a log bound above %g" % (
        name, 100 * share, R.UNCHECKED_AT))
    got, lg = _run_noise(impl, name, policy)
    _must("shape", lg.shape == r["log"].shape, lambda: "%s: %s" % (name, lg.shape))
    fig = dict(unchecked=share, worst=_within("spectrum", name, "spectrum", got, X, E))
    fig["log"] = _within("log", name, "log-power", lg, r["log"], r["dlog"], mask=r["checked"])
    got_s, sd = _run_noise(impl, name, policy, stats=True)
    _must("same-bits", np.array_equal(bits(got_s), bits(got)), "%s: the spectrum changes with the standardisation" % name)
    fig["std"] = _within("standardised", name, "standardised", sd, r["std"], r["dstd"], mask=r["checked"])
    fig["fro_log"], fig["fro_log_twin"] = R.rel_fro(lg, r["log"]), R.rel_fro(R.twin_features(chain, "log", cfg), r["log"])
    _note(tag, "features log", fig["log"], name)
    _note(tag, "features standardised", fig["std"], name)
    _log(tag, "%-22s %-6s features: worst error / bound log %.4f standardised %.4f; log features' relative Frobenius error %.3e "
         "(twin %.3e); unchecked %.4f %%" % (name, policy, fig["log"], fig["std"], fig["fro_log"], fig["fro_log_twin"], 100 * share))
    _must("aggregate", fig["fro_log"] <= R.TWIN_FACTOR * fig["fro_log_twin"], "%s: log features' relative Frobenius error %.3e, more than "
          "%g x the twin's %.3e" % (name, fig["fro_log"], R.TWIN_FACTOR, fig["fro_log_twin"]))
    _split_bits(impl, name, policy, ("std",), (got_s, sd), cache)
    return fig


def check_silence(impl, name, policy):
    c, cfg = CASES[name], cfg_of(CASES[name])
    got, lg = _run_noise(impl, name, policy)
    assert got.size > 0
    _must("zero", not (got != 0).any(), "%s: the spectrum of silence is not zero" % name)
    _must("silence", np.isfinite(lg).all() and R._ulps(lg, R.silence_log(c)).max() <= 2,
          lambda: "%s: log-power of silence is %r, expected %r" % (name, lg.flat[0], R.silence_log(c)))
    _, sd = _run_noise(impl, name, policy, stats=True)
    den = cfg["std"].astype(np.float64) + float(np.float32(cfg["norm_eps"]))
    sl = float(R.silence_log(c))
    ref = (sl - cfg["mean"].astype(np.float64)) / den
    _within("standardised", name, "standardised silence", sd, np.broadcast_to(ref, sd.shape),
            (2 * ULP * abs(sl) + ULP * np.abs(cfg["mean"])) / den + ULP * np.abs(ref))


# ------------------------------------------------------------------------------------------ direct calls and clamping
def direct_scenario(n_fft, hop, seed=0):
    """One call as a caller of the C entry point builds it, B = 3, 21 frames: row 0 has n_fft - hop pending samples and
    takes 7 hop more (7 frames, all but the last straddle), row 1 starts an utterance with n_fft + 6 hop + 3 samples (7 frames),
    row 2 has 5 pending, takes n_fft + 6 hop - 9 and ends (7 frames and the pad frame).  Impulses at least n_fft apart, at the
    ends of tail and chunk.  state_in holds NaN behind n_pending, the chunk behind n_valid.  -> keyword arguments of make_call"""
    rng = np.random.default_rng(seed + n_fft)
    pend, new, pad = [n_fft - hop, 0, 5], [7 * hop, n_fft + 6 * hop + 3, n_fft + 6 * hop - 9], [0, 0, 1]
    chunk = np.full((3, max(new)), np.nan, dtype=np.float32)
    state = np.full((3, n_fft), np.nan, dtype=np.float32)
    nf = []
    for b in range(3):
        Ls = pend[b] + new[b]
        x = np.zeros(Ls, dtype=np.float32)
        first = pend[b] if 0 < pend[b] < hop else 0       # row 2: the chunk's first sample, which a count beyond row 1's pitch would read
        for p in dict.fromkeys([first, max(pend[b] - 1, 0), pend[b], Ls - 1] + [int(v) for v in rng.integers(0, Ls, 6)]):
            if all(abs(p - q) >= n_fft for q in np.flatnonzero(x)):
                x[p] = float(rng.choice([-1.0, 1.0]) * 2.0 ** int(rng.integers(-6, 4)))
        state[b, :pend[b]], chunk[b, :new[b]] = x[:pend[b]], x[pend[b]:]
        nf.append((Ls - n_fft) // hop + 1 + pad[b])
    return dict(chunk=chunk, n_valid=new, n_pending=pend, n_frames=nf, pad=pad, state_in=state)


def _exact_call(tagname, name, call, g, c, tag=None):
    """one call of impulse data against ``ref_call``: shape, zero fill, state, then the exact tier on (frames / peak) @ basis64"""
    r = ref_call(call)
    try:
        check_call_shape(name, call, g, r)
        pk = np.ones(len(r["frames"])) if call["peak"] is None else call["peak"].astype(np.float64)
        fr = np.concatenate([f.astype(np.float64) / pk[b] for b, f in enumerate(r["frames"])], 0)
        ref = (fr @ R.basis64(c["n_fft"])).reshape(fr.shape[0], -1, 2)
        cat = lambda a: np.concatenate([a[b, :n[2]] for b, n in enumerate(r["counts"])], 0)
        _exact_tier(name, cat(g["spec"]), None if call["stats"] else cat(g["out"]), ref, c, tag)
    except AssertionError as e:
        if tagname is None:
            raise
        raise AssertionError("[%s] %s" % (tagname, e)) from None
    return r


def _same(tagname, a, b, msg):
    _must(tagname, all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("out", "spec", "state")), msg)


def check_direct(impl, n_fft, hop, tag="gpu"):
    c = dict(n_fft=n_fft, hop=hop, pad=True, fs=16e3, eps=1e-8, norm_eps=1e-3, name="direct-%dx%d" % (n_fft, hop))
    cfg = R.cfg_of(c)
    kw = direct_scenario(n_fft, hop)
    name, total, tmax = c["name"], sum(kw["n_frames"]), max(kw["n_frames"])
    base_call = make_call(cfg, **kw)
    base = impl(base_call)
    _exact_call(None, name, base_call, base, c, tag)
    for M in (0, 1, 10 * total):
        _same("hint-bits", impl(make_call(cfg, M=M, **kw)), base, "%s: d->M = %d changes a bit" % (name, M))
    wide = dict(kw, chunk=np.concatenate([kw["chunk"], np.full((3, 5), np.nan, dtype=np.float32)], 1))
    call = make_call(cfg, T=tmax + 3, **wide)
    g = impl(call)
    try:
        _exact_call(None, name + " T + 3, L + 5", call, g, c)
        _must("pitch", np.array_equal(bits(g["out"][:, :tmax]), bits(base["out"])) and np.array_equal(bits(g["spec"][:, :tmax]), bits(base["spec"]))
              and np.array_equal(bits(g["state"]), bits(base["state"])), "%s: larger pitches change a bit" % name)
    except AssertionError as e:
        raise AssertionError("[pitch] %s" % e) from None
    _same("peak-bits", impl(make_call(cfg, peak=np.ones(3, dtype=np.float32), **kw)), base, "%s: a peak of ones changes a bit" % name)
    for stats in (False, True):
        f = impl(make_call(cfg, spec=False, stats=stats, **kw))
        s = impl(make_call(cfg, spec=True, stats=stats, **kw))
        _must("same-bits", np.array_equal(bits(f["out"]), bits(s["out"])) and np.array_equal(bits(s["spec"]), bits(base["spec"])),
              "%s: fwd and fwd_spec differ (stats %s)" % (name, stats))


CLAMP_VARIANTS = ("frames+1+2", "valid+3", "pending+2", "negative", "pad-with-a-full-frame-left", "pad-frames+1")


def clamp_scenario(n_fft, hop, variant):
    """the direct scenario with counts that are wrong by small amounts; the pitches stay what the buffers hold"""
    kw = direct_scenario(n_fft, hop, seed=1)
    kw = dict(kw, n_valid=list(kw["n_valid"]), n_pending=list(kw["n_pending"]), n_frames=list(kw["n_frames"]), pad=list(kw["pad"]))
    T = max(kw["n_frames"])
    if variant == "frames+1+2":                           # rows that go on claim frames their samples do not complete
        kw["n_frames"][0] += 1
        kw["n_frames"][1] += 2
        T += 2
    elif variant == "valid+3":                            # the longest row claims 3 samples more than the pitch, and the frame they complete
        b = int(np.argmax(kw["n_valid"]))
        kw["chunk"] = kw["chunk"][:, :kw["n_valid"][b]]
        kw["n_valid"][b] += 3
        kw["n_frames"][b] = (kw["n_pending"][b] + kw["n_valid"][b] - n_fft) // hop + 1 + kw["pad"][b]
        T = max(T, max(kw["n_frames"]))
    elif variant == "pending+2":                          # a full state row (n_fft pending: the clamp's own limit) claimed as n_fft + 2
        st = kw["state_in"]
        st[0, :] = 0.0
        st[0, hop - 1] = 0.5                              # the chunk's first impulse lies at least n_fft behind it
        kw["n_pending"][0] = n_fft + 2
        kw["n_frames"][0] = (n_fft + 2 + kw["n_valid"][0] - n_fft) // hop + 1
        T = max(T, max(kw["n_frames"]))
    elif variant == "negative":
        kw["n_frames"][0], kw["n_pending"][1], kw["n_valid"][2] = -1, -2, -3
    elif variant == "pad-with-a-full-frame-left":         # pad_frames on a row that goes on: honest count, nothing changes
        kw["pad"][1] = 1
    else:
        assert variant == "pad-frames+1"                  # ... and with the frame the flag allows
        kw["pad"][1] = 1
        kw["n_frames"][1] += 1
        T = max(T, max(kw["n_frames"]))
    return kw, T


def check_clamp(impl, n_fft, hop, variant, tag="gpu"):
    """[clamp]: the outputs are those of the documented clamped counts; [guard]: the implementation's guard bands are intact"""
    c = dict(n_fft=n_fft, hop=hop, pad=True, fs=16e3, eps=1e-8, norm_eps=1e-3, name="clamp-%dx%d-%s" % (n_fft, hop, variant))
    cfg = R.cfg_of(c)
    kw, T = clamp_scenario(n_fft, hop, variant)
    call = make_call(cfg, T=T, M=0, arena=True, **kw)
    g = impl(call)
    r = _exact_call("clamp", c["name"], call, g, c, tag)
    bad = [n for n, ok in g.get("guards", []) if not ok]
    _must("guard", not bad, "%s: guard bands changed: %s" % (c["name"], bad))
    return r


# ------------------------------------------------------------------------------------------ the float32 CPU twin
MUTANTS = ("tail_late", "ignore_pending", "pad_reads_behind", "pad_not_final", "peak_multiplies", "no_scan_base", "skip_last_group",
           "last_bin_unwritten", "no_zero_fill", "idle_rewritten", "nvalid_unclamped", "f32_trig", "f32_trig_zeros", "imag_sign",
           "bf16_operands", "no_norm_eps")


def product_kernel_order(A, W, skip_last=False):
    """(M, K) x (K, N) float32 in the order of stream_product.h: wave w takes the groups kk = w, w + 8, ... (line 88), MFMA j of
    a group sums the four samples ``operand_index(K, kk, q, j)``, q = 0 .. 3, onto the accumulator; the eight partial sums are
    added in wave order (line 118).  All eight waves advance together here, a wave without a group adds zeros."""
    M, K = A.shape
    KQ = K // 16
    A0 = np.concatenate([A, np.zeros((M, 1), dtype=np.float32)], 1)
    W0 = np.concatenate([W, np.zeros((1, W.shape[1]), dtype=np.float32)], 0)
    acc = np.zeros((M, NW, W.shape[1]), dtype=np.float32)
    for g in range(-(-KQ // NW)):
        kks = [w + NW * g for w in range(NW)]
        live = [kk < KQ and not (skip_last and KQ % NW and kk == KQ - 1) for kk in kks]
        for j in range(4):
            s = None
            for q in range(4):
                ks = np.array([operand_index(K, kk, q, j) if ok else K for kk, ok in zip(kks, live)])
                t = A0[:, ks, None] * W0[ks][None]
                s = t if s is None else s + t
            acc += s
    v = acc[:, 0].copy()
    for w in range(1, NW):
        v += acc[:, w]
    assert v.dtype == np.float32
    return v


def make_twin(mutant=None, order="kernel"):
    assert mutant is None or mutant in MUTANTS

    def impl(call):
        cfg = call["cfg"]
        K, hop, T = cfg["n_fft"], cfg["hop"], call["T"]
        B, Lp = call["chunk"].shape
        F = K // 2 + 1
        flat = np.concatenate([call["chunk"].reshape(-1), np.full(K + 8, np.nan, dtype=np.float32)])
        sflat = np.concatenate([call["state_in"].reshape(-1), np.full(K + 8, np.nan, dtype=np.float32)])
        out = np.full((B, T, F), np.nan, dtype=np.float32)
        spec = np.full((B, T, F, 2), np.nan, dtype=np.float32)
        state = np.full((B, K), np.nan, dtype=np.float32)
        rows = []
        for b in range(B):                                # ss_row
            nv = max(call["n_valid"][b], 0) if mutant == "nvalid_unclamped" else _clamp(call["n_valid"][b], Lp)
            npd = _clamp(call["n_pending"][b], K)
            Ls = nv + npd
            cap = ((Ls - K) // hop + 1 if Ls >= K else 0) + (1 if call["pad"][b] or mutant == "pad_not_final" else 0)
            rows.append((nv, npd, _clamp(call["n_frames"][b], min(cap, T))))

        def sample(b, s, frame=False):                    # ss_sample on index arrays; frame: for a frame, not for the tail
            nv, npd, _ = rows[b]
            s = np.asarray(s)
            if mutant == "ignore_pending" and frame:
                pend = np.zeros(s.shape, dtype=np.float32)
            else:
                pend = sflat[np.clip(b * K + s, 0, sflat.size - 1)]
            c = s - npd
            inside = c < nv
            if mutant == "pad_reads_behind" and call["pad"][b] and frame:
                inside = np.ones_like(inside)
            new = np.where(inside, flat[np.clip(b * Lp + c, 0, flat.size - 1)], np.float32(0))
            return np.where(s < npd, pend, new).astype(np.float32)

        table, base = {}, 0                               # map_frames
        for c0 in range(0, B, 64):
            excl = 0 if mutant == "no_scan_base" else base
            for b in range(c0, min(c0 + 64, B)):
                for t in range(rows[b][2]):
                    table[excl + t] = (b, t)
                excl += rows[b][2]
                base += rows[b][2]
        slots = sorted(table.values())
        if slots:
            pk = np.ones(B, dtype=np.float32) if call["peak"] is None else call["peak"]
            A = np.stack([sample(b, t * hop + np.arange(K), frame=True) for b, t in slots])
            pks = np.array([pk[b] for b, _ in slots], dtype=np.float32)[:, None]
            A = (A * pks if mutant == "peak_multiplies" else A / pks).astype(np.float32)
            W = R._basis32(K, mutant if mutant in ("imag_sign", "f32_trig", "bf16_operands") else None)
            if mutant == "f32_trig_zeros":                # float32 trig and an unreduced phase, but the exact zeros forced
                W = np.where(R.basis64(K) == 0, np.float32(0), R._basis32(K, "f32_trig"))
            if mutant == "bf16_operands":
                A = R._to_bf16(A)
            with np.errstate(invalid="ignore", over="ignore"):
                X = R._chain(A, W) if order == "chain" else product_kernel_order(A, W, skip_last=mutant == "skip_last_group")
                re, im = X[:, 0::2], X[:, 1::2]
                pw = (re.astype(np.float64) ** 2 + (im * im).astype(np.float64)).astype(np.float32)      # fmaf(re, re, im * im)
                v = np.log((pw + np.float32(cfg["eps"])).astype(np.float64)).astype(np.float32)
                if call["stats"]:
                    den = cfg["std"] if mutant == "no_norm_eps" else cfg["std"] + np.float32(cfg["norm_eps"])
                    with np.errstate(divide="ignore"):
                        v = ((v - cfg["mean"]) / den).astype(np.float32)
            nbin = F - 1 if mutant == "last_bin_unwritten" else F
            for i, (b, t) in enumerate(slots):
                out[b, t, :nbin] = v[i, :nbin]
                spec[b, t, :nbin, 0], spec[b, t, :nbin, 1] = re[i, :nbin], im[i, :nbin]
        for b, (nv, npd, nf) in enumerate(rows):
            if mutant != "no_zero_fill":
                out[b, nf:], spec[b, nf:] = 0.0, 0.0
            if call["n_valid"][b] <= 0 and nf == 0:
                state[b] = 0.0 if mutant == "idle_rewritten" else call["state_in"][b]
                continue
            start = nf * hop + (1 if mutant == "tail_late" else 0)
            ln = min(max(npd + nv - start, 0), K)
            state[b] = 0.0
            state[b, :ln] = sample(b, start + np.arange(ln))
        return dict(out=out, spec=spec if call["spec"] else None, state=state)
    return impl
