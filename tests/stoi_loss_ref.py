"""Float64, differentiable restatement of the STOI / ESTOI training loss of include/avvad.h (avvad_stoi_loss,
csrc/stoi.hip) in torch on the CPU: the processed signal goes through stoi_ref's stages written as torch operations and
autograd gives the gradient of -d.  The cases, the taps, the keep decision (made from the clean signal, a constant here)
and the scores are stoi_ref's.

Beside it a hand-written chain (``manual_grad``): the closed forms of the header for a segment block and the adjoints of
the linear stages in numpy.  In float64 it must agree with autograd; with ``f32=True`` it is the float32 stand-in, the
same chain with float32 storage where the kernels round -- the resampled samples, the overlap-added samples, the ordered
float32 forward product, the dS operand, the ordered float32 adjoint product, the final gradient; and it carries the
mutants that the CPU tests use to show that the bound can fail.

The error of a gradient g against the float64 one is ``max|g - g64| / max|g64|`` per row.

The bounds.  MEASURED_STANDIN_GRAD is the stand-in's largest error over the gradient cases (``grad_cases``), measured on
the CPU by tests/test_stoi_loss_cpu.py, which prints the figure and holds the stand-in to GPU_GRAD_BOUND / 8 =
MEASURED_STANDIN_GRAD rounded up to two digits.  GPU_GRAD_BOUND is 8 times that: the margin this project gives a kernel
over its stand-in.  The yardstick is always the float64 reference.  The score itself keeps stoi_ref.GPU_BOUND.
MEASURED_STANDIN_CHAIN / GPU_CHAIN_BOUND are the same two figures for dlogits of the chain logits -> resynthesis -> loss
(``chain_case``), derived the same way.

Which cases.  The STOI gradient jumps where a clip decision flips, so it is compared only where the reference's smallest
relative clip gap |a y - C x| / (C x) is at least MIN_CLIP_GAP (about 100 times the float32 product's relative rounding);
the ESTOI gradient has no clip and is compared wherever there is a segment.
"""
import functools

import numpy as np
import torch

import stoi_ref as R

EPS = R.EPS
CLIP = 1.0 + 10.0 ** (R.BETA_DB / 20.0)
MIN_CLIP_GAP = 1e-4
NCOL = 2 * (R.F1 - R.F0)                      # 424 interleaved (re, im) columns

MEASURED_STANDIN_GRAD = 2.9e-6               # largest stand-in error over the gradient cases: 2.88e-6 (STOI of k16_11270), rounded up
GPU_GRAD_BOUND = 8 * MEASURED_STANDIN_GRAD
# The cases past one trip (stoi_ref.LONG_CASE_NAMES) have a constant of their own, by the same rule: the two 16 kHz rows of
# more than 1100 frames exceed the figure above (tests/test_stoi_long_cpu.py measures and prints every row).
MEASURED_STANDIN_GRAD_LONG = 3.3e-6          # largest stand-in error over the long cases: 3.26e-6 (STOI of k16_345004_both_sides), rounded up
GPU_GRAD_BOUND_LONG = 8 * MEASURED_STANDIN_GRAD_LONG


def grad_bound(name):
    """the GPU's bound on a case's gradient error"""
    return GPU_GRAD_BOUND_LONG if name in R.LONG_CASE_NAMES else GPU_GRAD_BOUND


# ---------------------------------------------------------------------------------------------- constants of the chain
@functools.lru_cache(maxsize=None)
def _resample_index(L):
    """the non-zero entries of the 5/8 resampler on L samples: (n, m, t) with out[n] += h[t] x[m], 8 n + 80 - t = 5 m"""
    n_out = -(-5 * L // 8)
    c = 8 * np.arange(n_out, dtype=np.int64) + 80
    ns, ms, ts = [], [], []
    for t in range(161):
        num = c - t
        ok = (num % 5 == 0) & (num >= 0) & (num < 5 * L)
        ns.append(np.nonzero(ok)[0]), ms.append(num[ok] // 5), ts.append(np.full(int(ok.sum()), t, dtype=np.int64))
    return n_out, np.concatenate(ns), np.concatenate(ms), np.concatenate(ts)


@functools.lru_cache(maxsize=None)
def basis64():
    """(256, 424) float64: column 2 j = w cos, 2 j + 1 = -w sin of bin 7 + j, the phase reduced exactly"""
    k = np.arange(R.N_FRAME, dtype=np.int64)[:, None]
    f = np.arange(R.F0, R.F1, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((f * k) % R.NFFT).astype(np.float64) / R.NFFT
    w = R.window()[:, None]
    out = np.empty((R.N_FRAME, NCOL))
    out[:, 0::2], out[:, 1::2] = w * np.cos(ang), -w * np.sin(ang)
    return out


@functools.lru_cache(maxsize=None)
def _band_of_column():
    """(424,) the band of every (re, im) column"""
    band = np.zeros(R.F1 - R.F0, dtype=np.int64)
    for j, (lo, hi) in enumerate(R.EDGES):
        band[lo - R.F0:hi - R.F0] = j
    return np.repeat(band, 2)


def clean_side(x, fs, f32=False):
    """what the clean signal fixes: (keep mask over the frames, X (15, M) band magnitudes, 10 kHz length)"""
    x = np.asarray(x, dtype=np.float64)
    x10 = R.resample(x, f32) if fs == 16000 else x
    mask = R.keep_mask(x10)
    xs = R.overlap_add(R.frames_of(x10, R.window())[mask])
    if f32:
        xs = xs.astype(np.float32).astype(np.float64)
    return mask, R.band_spectra(xs, f32=f32), x10.size


# ---------------------------------------------------------------------------------------------- the torch reference
def _unit_t(v, dim):
    v = v - v.mean(dim=dim, keepdim=True)
    return v / (torch.linalg.vector_norm(v, dim=dim, keepdim=True) + EPS)


def bands_torch(y, fs, mask):
    """processed samples (torch float64, at ``fs``) -> Y (15, M) through the resampler, the kept-frame overlap-add, the
    second framing and the banded DFT"""
    if fs == 16000:
        n_out, ni, mi, ti = _resample_index(y.numel())
        h = torch.from_numpy(R.taps())
        y = torch.zeros(n_out, dtype=torch.float64).index_add(0, torch.from_numpy(ni), h[torch.from_numpy(ti)] * y[torch.from_numpy(mi)])
    starts = R.frame_starts(y.numel())
    kept = starts[mask]
    if kept.size == 0:
        return torch.zeros((R.NUM_BANDS, 0), dtype=torch.float64)
    k = np.arange(R.N_FRAME)
    fr = torch.from_numpy(R.window())[None, :] * y[torch.from_numpy(kept[:, None] + k[None, :])]
    n = kept.size
    pos = torch.from_numpy((np.arange(n)[:, None] * R.HOP + k[None, :]).reshape(-1))
    sil = torch.zeros((n - 1) * R.HOP + R.N_FRAME, dtype=torch.float64).index_add(0, pos, fr.reshape(-1))
    st2 = R.frame_starts(sil.numel())
    if st2.size == 0:
        return torch.zeros((R.NUM_BANDS, 0), dtype=torch.float64)
    S = sil[torch.from_numpy(st2[:, None] + k[None, :])] @ torch.from_numpy(basis64())
    pw = (S * S).reshape(S.shape[0], -1, 2).sum(dim=2)
    return torch.stack([torch.sqrt(pw[:, lo - R.F0:hi - R.F0].sum(dim=1)) for lo, hi in R.EDGES])


def score_torch(X, Y, which):
    """d (a torch scalar) of the band magnitudes X (numpy, constant) and Y (torch), which 1 STOI, 2 ESTOI"""
    M = Y.shape[1]
    if M < R.N_SEG:
        return None
    xs = torch.from_numpy(R.segment_blocks(X))
    ys = torch.stack([Y[:, m - R.N_SEG:m] for m in range(R.N_SEG, M + 1)])
    if which == 1:
        nx, ny = (torch.linalg.vector_norm(v, dim=2, keepdim=True) for v in (xs, ys))
        yp = torch.minimum(nx / (ny + EPS) * ys, xs * CLIP)
        return torch.sum(_unit_t(xs, 2) * _unit_t(yp, 2)) / (xs.shape[0] * xs.shape[1])
    for dim in (2, 1):
        xs, ys = _unit_t(xs, dim), _unit_t(ys, dim)
    return torch.sum(xs * ys / R.N_SEG) / xs.shape[0]


def loss_and_grad(x, y, fs, which):
    """-> (d, gradient of -d in y at ``fs``) in float64 by autograd; a row without a segment: (1e-5, zeros)"""
    mask, X, _ = clean_side(x, fs)
    yt = torch.tensor(np.asarray(y, dtype=np.float64), requires_grad=True)
    d = score_torch(X, bands_torch(yt, fs, mask), which)
    if d is None:
        return R.DEGENERATE, np.zeros(yt.numel())
    (-d).backward()
    return float(d.detach()), yt.grad.numpy().copy()


def score_of(x, y, fs, which):
    """the float64 score alone (for finite differences)"""
    mask, X, _ = clean_side(x, fs)
    with torch.no_grad():
        d = score_torch(X, bands_torch(torch.tensor(np.asarray(y, dtype=np.float64)), fs, mask), which)
    return R.DEGENERATE if d is None else float(d)


# ---------------------------------------------------------------------------------------------- the closed forms
def unit_backward(v, g, axis, keep_mean=False):
    """the adjoint of u(v) = c / (n + eps), c = v - mean(v), n = |c| along ``axis`` under the cotangent g"""
    c = v - v.mean(axis=axis, keepdims=True)
    n = np.linalg.norm(c, axis=axis, keepdims=True)
    gc = np.sum(g * c, axis=axis, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        second = np.where(n != 0, c * gc / (n * (n + EPS) ** 2), 0.0)
    dc = g / (n + EPS) - second
    return dc if keep_mean else dc - dc.mean(axis=axis, keepdims=True)


def stoi_block_grad(xs, ys, no_mask=False, alpha_const=False, keep_mean=False):
    """gradient of -STOI in the (S, 15, 30) blocks ys (the header's closed form)"""
    S = xs.shape[0]
    nx, ny = np.linalg.norm(xs, axis=2, keepdims=True), np.linalg.norm(ys, axis=2, keepdims=True)
    alpha = nx / (ny + EPS)
    m = np.ones_like(ys) if no_mask else (alpha * ys < CLIP * xs).astype(np.float64)      # the tie is clipped
    p = np.minimum(alpha * ys, CLIP * xs)
    gp = unit_backward(p, -R._unit(xs, 2) / (R.NUM_BANDS * S), 2, keep_mean)
    dy = alpha * m * gp
    if not alpha_const:
        with np.errstate(divide="ignore", invalid="ignore"):
            dy = dy - np.where(ny != 0, nx * ys / (ny * (ny + EPS) ** 2), 0.0) * np.sum(m * gp * ys, axis=2, keepdims=True)
    return dy


def estoi_block_grad(xs, ys, keep_mean=False):
    S = xs.shape[0]
    xn = R._unit(R._unit(xs, 2), 1)
    g = unit_backward(R._unit(ys, 2), -xn / (R.N_SEG * S), 1, keep_mean)
    return unit_backward(ys, g, 2, keep_mean)


def clip_stats(X, Y):
    """-> (smallest relative clip gap |a y - C x| / (C x), clipped elements, elements) of STOI's blocks"""
    xs, ys = R.segment_blocks(X), R.segment_blocks(Y)
    alpha = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + EPS)
    gap = np.abs(alpha * ys - CLIP * xs) / (CLIP * xs)
    return float(gap.min()), int((alpha * ys >= CLIP * xs).sum()), int(xs.size)


# ---------------------------------------------------------------------------------------------- the hand-written chain
MUTANTS = ("no_clip_mask", "alpha_constant", "mean_kept", "segment_left_out", "resampler_shifted", "dropped_not_skipped")
# invert_kept answers -1 for frames >= 256 (its first workgroup alone ran): those frames lose their gradient in the
# overlap-add adjoint.  Only a row of more than 256 frames can tell.
LONG_MUTANTS = ("positions_of_one_block",)
INVERT_BLOCK = 256


def _chain32(A, Bm):
    """A (m, k) float32 times Bm (k, n) float32, one ordered float32 chain over k per value"""
    return R._chain32(np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(Bm, dtype=np.float32))


def manual_grad(x, y, fs, which, f32=False, mutant=None):
    """the gradient of -d in y by the closed forms and hand-written adjoints; ``f32``: the float32 stand-in"""
    assert mutant is None or mutant in MUTANTS or mutant in LONG_MUTANTS
    r32 = (lambda v: v.astype(np.float32).astype(np.float64)) if f32 else (lambda v: v)
    y = np.asarray(y, dtype=np.float64)
    mask, X, n10 = clean_side(x, fs, f32)
    y10 = R.resample(y, f32) if fs == 16000 else y
    w, k = R.window(), np.arange(R.N_FRAME)
    starts = R.frame_starts(n10)
    kept = starts[mask]
    M = kept.size - 1
    if M < R.N_SEG:
        return np.zeros(y.size)
    sil = r32(R.overlap_add(w[None, :] * y10[kept[:, None] + k[None, :]]))
    st2 = R.frame_starts(sil.size)
    assert st2.size == M
    raw = sil[st2[:, None] + k[None, :]]
    B64 = basis64()
    S = _chain32(raw, B64).astype(np.float64) if f32 else raw @ B64
    pw = (S * S).reshape(M, -1, 2).sum(axis=2)
    Y = np.stack([np.sqrt(pw[:, lo - R.F0:hi - R.F0].sum(axis=1)) for lo, hi in R.EDGES])
    xs, ys = R.segment_blocks(X), R.segment_blocks(Y)
    if which == 1:
        G = stoi_block_grad(xs, ys, mutant == "no_clip_mask", mutant == "alpha_constant", mutant == "mean_kept")
    else:
        G = estoi_block_grad(xs, ys, mutant == "mean_kept")
    nseg = G.shape[0]
    dY = np.zeros((R.NUM_BANDS, M))
    for s in range(nseg):                                          # ascending segments: the kernel's order
        if mutant == "segment_left_out" and s % 7 == 3:
            continue
        dY[:, s:s + R.N_SEG] += G[s]
    band = _band_of_column()
    with np.errstate(divide="ignore", invalid="ignore"):
        dS = np.where(Y.T[:, band] != 0, dY.T[:, band] * S / Y.T[:, band], 0.0)
    dfr = _chain32(dS, B64.T).astype(np.float64) if f32 else dS @ B64.T      # (_chain32 rounds dS on its way in)
    dsil = np.zeros(sil.size)
    np.add.at(dsil, st2[:, None] + k[None, :], dfr)
    dkept = dsil[np.arange(kept.size)[:, None] * R.HOP + k[None, :]] * w[None, :]
    dy10 = np.zeros(n10)
    if mutant == "positions_of_one_block":
        dkept[kept >= INVERT_BLOCK * R.HOP] = 0.0
    target = starts[:kept.size] if mutant == "dropped_not_skipped" else kept
    np.add.at(dy10, target[:, None] + k[None, :], dkept)
    if fs == 16000:
        _, ni, mi, ti = _resample_index(y.size)
        if mutant == "resampler_shifted":
            ti = np.minimum(ti + 1, 160)
        g = np.bincount(mi, weights=R.taps()[ti] * dy10[ni], minlength=y.size)
    else:
        g = dy10
    return r32(g)


def err(g, g64):
    """max|g - g64| / max|g64|"""
    g, g64 = np.asarray(g, dtype=np.float64), np.asarray(g64, dtype=np.float64)
    return float(np.max(np.abs(g - g64)) / np.max(np.abs(g64)))


# ---------------------------------------------------------------------------------------------- the shared references
@functools.lru_cache(maxsize=None)
def reference(name, which):
    """(d, gradient) of a stoi_ref case in float64, computed once; the gradient is read-only"""
    fs, x, y = R.case(name)
    d, g = loss_and_grad(x, y, fs, which)
    g.setflags(write=False)
    return d, g


@functools.lru_cache(maxsize=None)
def case_clip(name):
    """clip_stats of a case's float64 bands; None without a segment"""
    fs, x, y = R.case(name)
    mask, X, _ = clean_side(x, fs)
    with torch.no_grad():
        Y = bands_torch(torch.tensor(np.asarray(y, dtype=np.float64)), fs, mask).numpy()
    return clip_stats(X, Y) if Y.shape[1] >= R.N_SEG else None


def has_segment(name):
    return R.reference(name)["segments"] > 0


def grad_cases(which, names=R.CASE_NAMES):
    """the cases whose gradient is compared: every case with a segment for ESTOI; for STOI those whose clip gap allows it"""
    out = [n for n in names if has_segment(n)]
    return [n for n in out if case_clip(n)[0] >= MIN_CLIP_GAP] if which == 1 else out


def check_gradient(name, which, g):
    """What the GPU tests assert of a case's gradient g (L,) of -d: its shape, finite, exact zeros without a segment, and the
    error against float64 within grad_bound(name) wherever the gradient is compared.  -> the error, or None where it is not;
    the CPU tests hand it a mutant's gradient to show that it can fail."""
    g64 = reference(name, which)[1]
    g = np.asarray(g)
    key = "stoi" if which == 1 else "estoi"
    assert g.shape == g64.shape and np.isfinite(g).all()
    if not has_segment(name):
        assert not g.any()
        return None
    if name not in grad_cases(which, (name,)):
        print("%-22s %-5s gradient not compared: clip gap %.3g below %.3g" % (name, key, case_clip(name)[0], MIN_CLIP_GAP))
        return None
    e = err(g, g64)
    print("%-22s %-5s gradient error %.3g (bound %.3g), clipped %d of %d" % ((name, key, e, grad_bound(name)) + case_clip(name)[1:]))
    assert e <= grad_bound(name)
    return e


# ---------------------------------------------------------------------------------------------- the chain from the logits
MEASURED_STANDIN_CHAIN = 7.7e-7              # the stand-in's worst row of dlogits over chain_case(1), chain_case(2): 7.69e-7 (STOI), rounded up
GPU_CHAIN_BOUND = 8 * MEASURED_STANDIN_CHAIN


@functools.lru_cache(maxsize=None)
def chain_case(which, n_fft=1024, hop=256, sample_lengths=(11000, 9500), seed=41):
    """What a training step hands to ``ops.resynth`` (mask_mode 2) and ``ops.stoi_loss``: noisy / clean waves (B, L)
    zero-padded (stoi_ref.speech_pair, ungated, 5 dB), logits (B, T, F), ragged sample lengths, the first and last
    n_fft - hop samples of every row left out by slicing.  Holds dlogits in float64 (sisdr_ref's differentiable inverse,
    then this module's chain, autograd through both) and the float32 stand-in (istft_ref's float32 GEMM forms around
    ``manual_grad(f32=True)``), with each row's keep margin and clip statistics of the float64 chain."""
    import istft_ref as I
    import sisdr_ref as S
    from avvad import ops              # (host-side frame arithmetic only)
    rng = np.random.default_rng(seed)
    B, L, F = len(sample_lengths), max(sample_lengths), n_fft // 2 + 1
    frames = [ops.n_frames(n, n_fft, hop) for n in sample_lengths]
    T = max(frames)
    noisy, clean = np.zeros((B, L), dtype=np.float32), np.zeros((B, L), dtype=np.float32)
    for b, n in enumerate(sample_lengths):
        clean[b, :n], noisy[b, :n] = R.speech_pair(seed + 1 + b, n, 16000, 5.0, 0.0)
    logits = (rng.standard_normal((B, T, F)) * 1.5).astype(np.float32)
    skip = n_fft - hop
    case = dict(n_fft=n_fft, hop=hop, start=0, center=False, mode=2, frames=frames, lengths=list(sample_lengths), noisy=noisy,
                clean=clean, mask=logits, skip=skip, scale=None, which=which)
    spec64 = np.zeros((B, T, F, 2))
    for b, n in enumerate(sample_lengths):
        Sb = I.stft64(noisy[b, :n], n_fft, hop)
        assert Sb.shape[0] == frames[b]
        spec64[b, :frames[b], :, 0], spec64[b, :frames[b], :, 1] = Sb.real, Sb.imag
    c64 = dict(case, spec=spec64, dout=np.zeros((B, L)))
    lt = torch.from_numpy(logits.astype(np.float64)).requires_grad_(True)
    loss = torch.zeros((), dtype=torch.float64)
    case["d64"], case["margin"], case["clip"] = [], [], []
    for b, yrow in enumerate(S.est64(c64, lt)):
        n = sample_lengths[b]
        yrow = torch.nn.functional.pad(yrow, (0, n - yrow.numel()))
        xin = clean[b, skip:n - skip]
        mask, X, _ = clean_side(xin, 16000)
        Y = bands_torch(yrow[skip:n - skip], 16000, mask)
        d = score_torch(X, Y, which)
        loss = loss - d
        case["d64"].append(float(d.detach()))
        case["margin"].append(R.margin(xin, 16000))
        case["clip"].append(clip_stats(X, Y.detach().numpy()))
    loss.backward()
    case["loss64"], case["ref"] = float(loss.detach()), lt.grad.numpy()
    spec32 = np.zeros((B, T, F, 2), dtype=np.float32)
    g32 = np.zeros((B, L), dtype=np.float32)
    for b, n in enumerate(sample_lengths):
        A = I.stft32_gemm(noisy[b, :n], n_fft, hop)
        spec32[b, :frames[b], :, 0], spec32[b, :frames[b], :, 1] = A[:, 0::2], A[:, 1::2]
        sg = (1.0 / (1.0 + np.exp(-logits[b, :frames[b]]))).astype(np.float32)
        est = I.istft32_gemm(A * np.repeat(sg, 2, axis=1), n_fft, hop, length=n)
        g32[b, skip:n - skip] = manual_grad(clean[b, skip:n - skip], est[skip:n - skip], 16000, which, f32=True)
    case["y32"] = S.dmask_closed(dict(case, spec=spec32, dout=g32), np.float32)
    return case


def chain_err(got, case):
    """the worst row's max|g - g64| / max|g64| of dlogits (B, T, F)"""
    return max(err(np.asarray(got)[b], case["ref"][b]) for b in range(case["ref"].shape[0]))
