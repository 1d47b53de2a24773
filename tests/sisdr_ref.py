"""The oracle of the SI-SDR training path: the adjoint of the masked inverse STFT with respect to the mask (or its logits)
and the SI-SDR loss with its gradient.  Three evaluations of the same chain:

* the float64 reference -- torch on the CPU: spectrum x g(mask), per-frame ``irfft``, Hann, overlap-add, the ``> tiny``
  division, crop, the reference's ``energy_ratios`` formula; gradients from autograd (``dmask64``, ``sisdr64``,
  ``chain_case``);
* the closed forms -- the adjoint identity and the two-coefficient gradient as plain numpy (``dmask_closed``,
  ``sisdr_closed``), in the GEMM form the GPU uses (matrix products against the bases of ``istft_ref``, not an FFT);
  evaluated in float64 they must equal autograd, and a ``Form`` switches single terms off to make the mutants the
  assertion functions have to reject;
* the float32 yardstick -- the closed forms evaluated in float32 (the inner products of the loss in double, as the
  kernel has them): ``E_cpu32 = max |yardstick - float64|`` is the error a float32 GEMM form makes on these inputs, and
  the bound of a GPU result is ``istft_ref.FACTOR * E_cpu32``.

The assertion functions (``check_dmask``, ``check_sisdr``, ``check_chain``) take an implementation callable -- the GPU op
in tests/test_sisdr_gpu.py, the closed forms and their mutants in tests/test_sisdr_cpu.py."""
import functools

import numpy as np
import torch

import istft_ref as R

K10 = 20.0 / np.log(10.0)
GRAD_EPS = 2.0 ** -21          # c1 s + c2 e in float32: two rounded coefficients, two products, one sum: <= 3 * 2^-24


class Form:
    """what a closed form computes; the defaults are the mathematics, every other value a mutant"""
    zero_rows = True           # frames t >= n_frames[b] of dmask are zero
    edge_weight = 1.0          # w_f of DC and Nyquist
    inv_n = True               # the 1 / N of the inverse basis
    cut_at_len = True          # q is zero at and behind out_len[b]
    use_scale = True           # q carries scale[b]
    sin_sign = -1.0            # the imaginary basis is -sin
    full_c1 = True             # c1 holds its a / (r D) term
    use_tail = True            # the loss window ends skip_tail samples before the row's length

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(Form, k), k
            setattr(self, k, v)


MUTANTS = {
    "rows t >= n_frames not zeroed": Form(zero_rows=False),
    "w_f = 2 at DC and Nyquist": Form(edge_weight=2.0),
    "1/N dropped": Form(inv_n=False),
    "q not cut at out_len": Form(cut_at_len=False),
    "scale left out of q": Form(use_scale=False),
    "+sin in place of -sin": Form(sin_sign=1.0),
}
LOSS_MUTANTS = {
    "c1 without a/(rD)": Form(full_c1=False),
    "tail skip ignored": Form(use_tail=False),
}


# ------------------------------------------------------------------------------------------------ the masked inverse
def forward_basis(n_fft, sin_sign=-1.0):
    """(n_fft, 2F) float64: column 2f = hann cos, 2f + 1 = -hann sin (the basis of ``istft_ref.stft32_gemm``)"""
    F = n_fft // 2 + 1
    k, f = np.arange(n_fft)[:, None], np.arange(F)[None, :]
    ang = 2.0 * np.pi * ((f * k) % n_fft) / n_fft
    W = np.empty((n_fft, 2 * F))
    W[:, 0::2] = R.hann(n_fft)[:, None] * np.cos(ang)
    W[:, 1::2] = sin_sign * R.hann(n_fft)[:, None] * np.sin(ang)
    return W


def _wss(nf, n_fft, hop, Lq):
    """window sum of squares of a row of nf frames over Lq samples, ascending in double as the kernels add it"""
    w2 = R.hann(n_fft) ** 2
    wss = np.zeros(Lq)
    for t in range(nf):
        wss[t * hop:t * hop + n_fft] += w2
    return wss


def _valid(case, b, cut_at_len=True):
    """samples of row b the forward wrote a sum to"""
    nf = case["frames"][b]
    natural = case["n_fft"] + case["hop"] * (nf - 1) - case["start"] if nf > 0 else 0
    pitch = case["dout"].shape[1]
    return max(0, min(min(case["lengths"][b], pitch) if cut_at_len else pitch, natural))


def dmask_closed(case, dtype=np.float64, form=None):
    """The adjoint in the GEMM form: q, G = frames(q) @ forward basis, dmask = (w_f / N)(G_re S_re + G_im S_im)
    [sigmoid'].  ``dtype`` float64: the closed form; float32: the yardstick (every product and sum in float32, the window
    sum as the float the forward divides by)."""
    form = form or Form()
    N, hop, start, mode = case["n_fft"], case["hop"], case["start"], case["mode"]
    spec, mask, dout = case["spec"], case["mask"], case["dout"]
    B, T, F = mask.shape
    Lq = (T - 1) * hop + N
    W = forward_basis(N, form.sin_sign).astype(dtype)
    wf = np.full(F, 2.0)
    wf[0] = wf[N // 2] = form.edge_weight
    wf = (wf / N if form.inv_n else wf).astype(dtype)
    out = np.zeros((B, T, F), dtype=dtype)
    for b in range(B):
        nf = case["frames"][b]
        n = _valid(case, b, form.cut_at_len)
        wss = _wss(nf, N, hop, Lq)
        w = wss if dtype == np.float64 else wss.astype(np.float32)
        q = np.zeros(Lq, dtype=dtype)
        g = dout[b, :n].astype(dtype)
        if case["scale"] is not None and form.use_scale:
            g = g * dtype(case["scale"][b])
        wv = w[start:start + n]
        q[start:start + n] = np.where(wv > R.TINY32, g / np.where(wv > R.TINY32, wv, 1).astype(dtype), g)
        G = np.stack([q[t * hop:t * hop + N] for t in range(T)]) @ W
        rows = nf if form.zero_rows else T
        S = spec[b, :rows].astype(dtype)
        m = mask[b, :rows].astype(dtype)
        if not form.zero_rows:                                  # (the padding holds NaN: the mutant is "q's transform alone")
            S[nf:], m[nf:] = 1.0, 0.5
        d = wf * (G[:rows, 0::2] * S[:, :, 0] + G[:rows, 1::2] * S[:, :, 1])
        if mode == 2:
            sg = (1.0 / (1.0 + np.exp(-m))).astype(dtype)
            d = d * (sg * (1 - sg))
        out[b, :rows] = d
    return out


def _inverse64(S, g, n_fft, hop, start, n, scale):
    """torch float64: masked spectrum (nf, F) complex -> the n output samples of the forward (irfft, Hann, overlap-add,
    the > tiny division, trim, scale)"""
    nf = S.shape[0]
    fr = torch.fft.irfft(S * g, n=n_fft, dim=1) * torch.from_numpy(R.hann(n_fft))
    Lq = (nf - 1) * hop + n_fft
    num = torch.zeros(Lq, dtype=torch.float64)
    for t in range(nf):
        num = num + torch.nn.functional.pad(fr[t], (t * hop, Lq - t * hop - n_fft))
    wss = torch.from_numpy(_wss(nf, n_fft, hop, Lq))
    y = torch.where(wss > R.TINY32, num / torch.where(wss > R.TINY32, wss, torch.ones_like(wss)), num)
    return y[start:start + n] * scale


def est64(case, mask_t):
    """list of the rows' valid samples as float64 torch tensors, differentiable in ``mask_t`` (B, T, F) float64"""
    rows = []
    for b, nf in enumerate(case["frames"]):
        n = _valid(case, b)
        if nf == 0 or n == 0:
            rows.append(torch.zeros(0, dtype=torch.float64))
            continue
        S = torch.from_numpy(case["spec"][b, :nf].astype(np.float64))
        S = torch.complex(S[..., 0], S[..., 1])
        m = mask_t[b, :nf]
        g = torch.sigmoid(m) if case["mode"] == 2 else m
        sc = 1.0 if case["scale"] is None else float(case["scale"][b])
        rows.append(_inverse64(S, g, case["n_fft"], case["hop"], case["start"], n, sc))
    return rows


def dmask64(case):
    """float64 autograd: d <out, dout> / d mask, zero in the padding frames"""
    mask = np.nan_to_num(case["mask"].astype(np.float64))       # (the padding is never used: est64 slices it off)
    mt = torch.from_numpy(mask).requires_grad_(True)
    tot = 0.0
    for b, y in enumerate(est64(case, mt)):
        tot = tot + (y * torch.from_numpy(case["dout"][b, :y.numel()].astype(np.float64))).sum()
    tot.backward()
    return mt.grad.numpy()


def istft_case(n_fft, hop, frames, mode, center, seed, lengths=None, scale=None, spec_rows=None):
    """A ragged batch for the adjoint: random spectra (or ``spec_rows``, a list of (>= frames[b], F, 2) float32 arrays; NaN
    in the padding frames either way), a mask in [0, 1) (mode 1) or logits
    (mode 2) with NaN in the padding, a normal cotangent with NaN behind each row's length -- with ``center`` a full one,
    without it zero in the first and last n_fft - hop samples of every row, where the window sum of squares falls to
    1e-10.  A row of 0 frames is all padding, has length 0 and a zero row in the reference.  Holds the float64 reference
    and the float32 yardstick of dmask."""
    rng = np.random.default_rng(seed)
    B, T, F = len(frames), max(frames), n_fft // 2 + 1
    start = n_fft // 2 if center else 0
    spec = np.full((B, T, F, 2), np.nan, dtype=np.float32)
    mask = np.full((B, T, F), np.nan, dtype=np.float32)
    nat = [R.istft_length(nf, n_fft, hop, center) for nf in frames]
    lens = list(nat) if lengths is None else list(lengths)
    dout = np.full((B, max(lens)), np.nan, dtype=np.float32)
    for b, nf in enumerate(frames):
        if spec_rows is None:
            if nf > 0:                                          # (a row of 0 frames is all padding: NaN, and a zero row of dmask)
                S = R.random_spectrum(rng, nf, n_fft)
                spec[b, :nf, :, 0], spec[b, :nf, :, 1] = S.real, S.imag
        else:
            spec[b, :nf] = spec_rows[b][:nf]
        mask[b, :nf] = rng.random((nf, F)) if mode == 1 else rng.standard_normal((nf, F)) * 2.0
        n = min(lens[b], nat[b])
        d = rng.standard_normal(lens[b]).astype(np.float32)
        if not center:
            edge = n_fft - hop
            d[:edge] = 0.0
            d[max(0, n - edge):] = 0.0
        dout[b, :lens[b]] = d
    case = dict(n_fft=n_fft, hop=hop, start=start, center=center, mode=mode, frames=list(frames), lengths=lens, spec=spec, mask=mask,
                dout=dout, scale=None if scale is None else np.asarray(scale, dtype=np.float32))
    case["ref"] = dmask64(case)
    case["y32"] = dmask_closed(case, np.float32)
    return case


@functools.lru_cache(maxsize=None)
def cached_istft_case(*a, **k):
    return istft_case(*a, **k)


def check_dmask(impl, case, report=None, name="dmask"):
    """``impl(case)`` -> dmask (B, T, F): finite, exactly zero for t >= n_frames[b], within FACTOR x E_cpu32 of float64"""
    got = np.asarray(impl(case))
    ref, y32 = case["ref"], case["y32"]
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), name + ": non-finite values"
    for b, nf in enumerate(case["frames"]):
        assert not got[b, nf:].any() and not np.signbit(got[b, nf:]).any(), "%s: row %d is not zero from frame %d" % (name, b, nf)
    e32 = float(np.abs(y32.astype(np.float64) - ref).max())
    e = float(np.abs(got.astype(np.float64) - ref).max())
    assert e32 > 0
    print("sisdr: %-52s E = %.3e  E_cpu32 = %.3e  ratio %.2f" % (name, e, e32, e / e32))
    if report is not None:
        report(name, got.astype(np.float64), ref, R.FACTOR * e32)
    assert e <= R.FACTOR * e32, "%s: E = %.3e above %g x E_cpu32 = %.3e" % (name, e, R.FACTOR, R.FACTOR * e32)
    return e, e32


# ------------------------------------------------------------------------------------------------ the loss
def _window(lengths, L, head, tail, use_tail=True):
    return [(min(head, L), max(min(head, L), min(n, L) - (tail if use_tail else 0))) for n in lengths]


def sisdr_closed(est, ref, lengths, head=0, tail=0, dtype=np.float64, form=None):
    """(loss, ratios (B,), grad (B, L), c1 (B,), c2 (B,)): the sums a, r, e in double, the two coefficients in double (rounded
    to ``dtype``), grad = c1 ref + c2 est in ``dtype`` inside the window and zero outside; an empty window adds nothing."""
    form = form or Form()
    est, ref = np.asarray(est), np.asarray(ref)
    B, L = est.shape
    grad = np.zeros((B, L), dtype=dtype)
    ratios, c1s, c2s = np.full(B, np.nan), np.zeros(B), np.zeros(B)
    loss = 0.0
    for b, (lo, hi) in enumerate(_window(lengths, L, head, tail, form.use_tail)):
        if hi <= lo:
            continue
        e, s = est[b, lo:hi].astype(np.float64), ref[b, lo:hi].astype(np.float64)
        a, r, ee = float(e @ s), float(s @ s), float(e @ e)
        D = ee - a * a / r
        ratios[b] = 10.0 * np.log10((a * a / r) / D)
        c1s[b] = -K10 * (1.0 / a + (a / (r * D) if form.full_c1 else 0.0))
        c2s[b] = K10 / D
        grad[b, lo:hi] = dtype(c1s[b]) * ref[b, lo:hi].astype(dtype) + dtype(c2s[b]) * est[b, lo:hi].astype(dtype)
        loss -= ratios[b]
    return loss, ratios, grad, c1s, c2s


def _energy_ratio64(e, s):
    """the reference's ``energy_ratios`` SI-SDR of one row: 10 log10 |alpha s|^2 / |e - alpha s|^2, torch float64"""
    alpha = (e * s).sum() / (s * s).sum()
    target = alpha * s
    return 10.0 * torch.log10((target * target).sum() / ((e - target) ** 2).sum())


def sisdr64(est, ref, lengths, head=0, tail=0):
    """float64 autograd: (loss, ratios (B,), grad (B, L))"""
    et = torch.from_numpy(np.nan_to_num(np.asarray(est, dtype=np.float64))).requires_grad_(True)
    rt = torch.from_numpy(np.nan_to_num(np.asarray(ref, dtype=np.float64)))
    ratios = np.full(et.shape[0], np.nan)
    loss = torch.zeros((), dtype=torch.float64)
    for b, (lo, hi) in enumerate(_window(lengths, et.shape[1], head, tail)):
        if hi > lo:
            v = _energy_ratio64(et[b, lo:hi], rt[b, lo:hi])
            ratios[b] = float(v.detach())
            loss = loss - v
    if loss.requires_grad:
        loss.backward()
    grad = et.grad.numpy() if et.grad is not None else np.zeros(et.shape)
    return float(loss.detach()), ratios, grad


def check_sisdr(impl, case, name="si_sdr_loss"):
    """``impl(case)`` -> (loss, ratios (B,), grad (B, L)).  Values within 1e-6 dB per row of float64 (rows between -10 and
    60 dB), the gradient element-wise within 2^-21 (|c1 s| + |c2 e|) of the float64 coefficients, exact zeros outside the
    window, an empty window: zero loss, zero gradient, no NaN."""
    est, ref, lengths, head, tail = case["est"], case["ref"], case["lengths"], case["head"], case["tail"]
    loss, ratios, grad = impl(case)
    grad, ratios = np.asarray(grad), np.asarray(ratios, dtype=np.float64)
    loss64, ratios64, grad64 = case["ref64"]
    _, _, _, c1, c2 = sisdr_closed(est, ref, lengths, head, tail)
    assert grad.shape == est.shape and np.isfinite(grad).all() and np.isfinite(loss), name + ": non-finite values"
    for b, (lo, hi) in enumerate(_window(lengths, est.shape[1], head, tail)):
        out = np.concatenate([grad[b, :lo], grad[b, max(hi, lo):]])
        assert not out.any() and not np.signbit(out).any(), "%s: row %d has a gradient outside its window" % (name, b)
        if hi <= lo:
            continue
        assert -10 <= ratios64[b] <= 60
        print("sisdr: %-40s row %d  %.6f dB  |d| = %.2e dB" % (name, b, ratios[b], abs(ratios[b] - ratios64[b])))
        assert abs(ratios[b] - ratios64[b]) <= 1e-6, (b, ratios[b], ratios64[b])
        mag = np.abs(c1[b] * ref[b, lo:hi].astype(np.float64)) + np.abs(c2[b] * est[b, lo:hi].astype(np.float64))
        err = np.abs(grad[b, lo:hi].astype(np.float64) - grad64[b, lo:hi])
        worst = float((err / np.maximum(mag, 1e-300)).max())
        print("sisdr: %-40s row %d  gradient max err / (|c1 s| + |c2 e|) = %.2e (bound %.2e)" % (name, b, worst, GRAD_EPS))
        assert (err <= GRAD_EPS * mag).all(), (b, worst)
    n_rows = sum(1 for lo, hi in _window(lengths, est.shape[1], head, tail) if hi > lo)
    assert abs(loss - loss64) <= 1e-6 * max(n_rows, 1) + 2.0 ** -23 * abs(loss64), (loss, loss64)     # (the loss is a float32)
    return loss, ratios, grad


def sisdr_case(lengths, L, head, tail, seed, snr_db=(5.0, 20.0)):
    """est / ref (B, L) float32: a clean signal plus noise at ``snr_db`` (cycled over the rows), NaN at and behind each
    row's length"""
    rng = np.random.default_rng(seed)
    B = len(lengths)
    est = np.full((B, L), np.nan, dtype=np.float32)
    ref = np.full((B, L), np.nan, dtype=np.float32)
    for b, n in enumerate(lengths):
        s = rng.standard_normal(n) * 0.1
        noise = rng.standard_normal(n) * 0.1 * 10.0 ** (-snr_db[b % len(snr_db)] / 20.0)
        ref[b, :n] = s
        est[b, :n] = 0.7 * s + noise
    case = dict(est=est, ref=ref, lengths=list(lengths), head=head, tail=tail)
    case["ref64"] = sisdr64(est, ref, lengths, head, tail)
    return case


# ------------------------------------------------------------------------------------------------ the whole chain
def chain_case(n_fft, hop, sample_lengths, seed, scale=None):
    """noisy / clean waves (B, L) zero-padded, logits (B, T, F), ragged sample lengths: what a training step hands to
    ``ops.resynth`` (mask_mode 2) and ``ops.si_sdr_loss`` (skips n_fft - hop).  Holds dlogits in float64 (autograd through
    the whole chain) and in the float32 GEMM form."""
    from avvad import ops              # (host-side frame arithmetic only)
    rng = np.random.default_rng(seed)
    B, L, F = len(sample_lengths), max(sample_lengths), n_fft // 2 + 1
    frames = [ops.n_frames(n, n_fft, hop) for n in sample_lengths]
    T = max(frames)
    noisy, clean = np.zeros((B, L), dtype=np.float32), np.zeros((B, L), dtype=np.float32)
    for b, n in enumerate(sample_lengths):
        t = np.arange(n) / 16e3
        s = 0.5 * np.sin(2 * np.pi * (220.0 + 110.0 * b) * t) * (1.0 + 0.5 * np.sin(2 * np.pi * 3.0 * t)) + 0.05 * rng.standard_normal(n)
        clean[b, :n] = s
        noisy[b, :n] = s + 0.3 * rng.standard_normal(n)
    logits = (rng.standard_normal((B, T, F)) * 1.5).astype(np.float32)
    skip = n_fft - hop
    case = dict(n_fft=n_fft, hop=hop, start=0, center=False, mode=2, frames=frames, lengths=list(sample_lengths), noisy=noisy,
                clean=clean, mask=logits, skip=skip, scale=None if scale is None else np.asarray(scale, dtype=np.float32))
    # float64: the spectrum of each row's own samples (with its end pad), the inverse, the windowed loss, autograd
    spec64 = np.zeros((B, T, F, 2))
    for b, n in enumerate(sample_lengths):
        S = R.stft64(noisy[b, :n], n_fft, hop)
        assert S.shape[0] == frames[b]
        spec64[b, :frames[b], :, 0], spec64[b, :frames[b], :, 1] = S.real, S.imag
    c64 = dict(case, spec=spec64, dout=np.zeros((B, L)))
    lt = torch.from_numpy(logits.astype(np.float64)).requires_grad_(True)
    loss = torch.zeros((), dtype=torch.float64)
    for b, y in enumerate(est64(c64, lt)):
        n = sample_lengths[b]
        y = torch.nn.functional.pad(y, (0, n - y.numel()))
        loss = loss - _energy_ratio64(y[skip:n - skip], torch.from_numpy(clean[b, skip:n - skip].astype(np.float64)))
    loss.backward()
    case["loss64"], case["ref"] = float(loss), lt.grad.numpy()
    # float32 GEMM form: forward transform, masked inverse, sums in double, gradient, adjoint
    spec32 = np.zeros((B, T, F, 2), dtype=np.float32)
    est32 = np.zeros((B, L), dtype=np.float32)
    for b, n in enumerate(sample_lengths):
        A = R.stft32_gemm(noisy[b, :n], n_fft, hop)
        spec32[b, :frames[b], :, 0], spec32[b, :frames[b], :, 1] = A[:, 0::2], A[:, 1::2]
        sg = (1.0 / (1.0 + np.exp(-logits[b, :frames[b]]))).astype(np.float32)
        y = R.istft32_gemm(A * np.repeat(sg, 2, axis=1), n_fft, hop, length=n)
        est32[b, :n] = y if scale is None else y * np.float32(scale[b])
    _, _, g32, _, _ = sisdr_closed(est32, clean, sample_lengths, skip, skip, dtype=np.float32)
    case["y32"] = dmask_closed(dict(case, spec=spec32, dout=g32), np.float32)
    return case


def check_chain(impl, case, report=None, name="chain"):
    """``impl(case)`` -> (loss, dlogits (B, T, F)) under the FACTOR x E_cpu32 bound of dlogits"""
    loss, got = impl(case)
    print("sisdr: %-52s loss %.6f  float64 %.6f" % (name, loss, case["loss64"]))
    assert np.isfinite(loss)
    return check_dmask(lambda c: got, case, report, name)
