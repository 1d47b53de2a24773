"""Float64 numpy statement of the scores of csrc/scores.hip, written from the formulas (not from the kernel):

  alphas / components / energy_ratios    the reference's projections: alpha_s = <e, s> / |s|^2, alpha_n = <e, n> / |n|^2,
                                         s_target = alpha_s s, e_noise = alpha_n n, e_art = e - s_target - e_noise, and
                                         10 log10 of |s_target|^2 over |e_noise + e_art|^2, |e_noise|^2, |e_art|^2, with
                                         the planes formed and their norms taken -- the long way round
  gram_ratios(..., chunk)                the closed form in the six inner products, each summed the way the kernel sums:
                                         per chunk 256 lanes striding over it, the lanes added, the chunks ascending
  confusion                              tp, tn, fp, fn as integers
  draw / many_chunk_lengths              the signals the CPU and GPU tests share: a draw whose every ratio lies in [-10, 60] dB,
                                         and the five row lengths of 8 to 17 chunks at which the finishing kernel's unrolled
                                         sum of a row's partials (add_ascending<8>) runs its body, body + remainder

pinned by tests/golden/scores.npz (tools/gen_golden.py scores: the reference's own functions on the same inputs).
A plain module: no fixtures."""
import numpy as np

LANES = 256
GAINS = (1.0, 0.1, 1e-3)
ART_DB = (0.0, 20.0, 40.0)


def _f64(*xs):
    return [np.asarray(x, dtype=np.float64).reshape(-1) for x in xs]


def alphas(s_hat, s, n):
    e, s, n = _f64(s_hat, s, n)
    with np.errstate(all="ignore"):
        return np.dot(e, s) / np.dot(s, s), np.dot(e, n) / np.dot(n, n)


def components(s_hat, s, n):
    e, s, n = _f64(s_hat, s, n)
    a_s, a_n = alphas(e, s, n)
    s_target, e_noise = a_s * s, a_n * n
    return s_target, e_noise, e - s_target - e_noise


def _db(num, den):
    with np.errstate(all="ignore"):
        return 10.0 * np.log10(np.float64(num) / np.float64(den))


def energy_ratios(s_hat, s, n=None):
    """(si_sdr, si_sir, si_sar) in dB; n None: SI-SDR alone, the other two NaN.  An empty signal gives NaN."""
    if n is None:
        e, s = _f64(s_hat, s)
        with np.errstate(all="ignore"):
            t = np.dot(e, s) / np.dot(s, s) * s
        return _db(np.dot(t, t), np.dot(e - t, e - t)), np.nan, np.nan
    s_target, e_noise, e_art = components(s_hat, s, n)
    res = e_noise + e_art
    p = np.dot(s_target, s_target)
    return _db(p, np.dot(res, res)), _db(p, np.dot(e_noise, e_noise)), _db(p, np.dot(e_art, e_art))


def _chunked_dot(a, b, chunk):
    total = np.float64(0.0)
    for i0 in range(0, a.size, chunk):
        p = a[i0:i0 + chunk] * b[i0:i0 + chunk]
        lanes = np.zeros(LANES)
        for l in range(min(LANES, p.size)):
            lanes[l] = np.add.reduce(p[l::LANES])           # (numpy may pair these; the order inside a lane is not pinned)
        total += lanes.sum()
    return total


def gram_ratios(s_hat, s, n, chunk=4096):
    """The three ratios from G = (e.e, e.s, e.n, s.s, n.n, s.n) with chunked double sums."""
    e, s, n = _f64(s_hat, s, n)
    ee, es, en = _chunked_dot(e, e, chunk), _chunked_dot(e, s, chunk), _chunked_dot(e, n, chunk)
    ss, nn, sn = _chunked_dot(s, s, chunk), _chunked_dot(n, n, chunk), _chunked_dot(s, n, chunk)
    with np.errstate(all="ignore"):
        a_s, a_n = es / ss, en / nn
    target, noise = a_s * es, a_n * en
    clamp = lambda d: d if not d < 0 else 0.0               # noqa: E731
    return (_db(target, clamp(ee - target)), _db(target, noise),
            _db(target, clamp(ee - target - noise + 2.0 * a_s * a_n * sn)))


def confusion(pred_hard, target, lengths=None):
    """(B, 4) int64 tp, tn, fp, fn over the frames t < lengths[b] of pred_hard / target (B, T, ...) holding 0 / 1."""
    B = pred_hard.shape[0]
    out = np.zeros((B, 4), dtype=np.int64)
    for b in range(B):
        n = pred_hard.shape[1] if lengths is None else int(lengths[b])
        p, y = np.asarray(pred_hard[b, :n]).astype(bool), np.asarray(target[b, :n]).astype(bool)
        out[b] = [(p & y).sum(), (~p & ~y).sum(), (p & ~y).sum(), (~p & y).sum()]
    return out


def mix(rng, L, g, art_db, dtype=np.float32):
    """The test signals: s_hat = 0.7 s + g n + e with e ``art_db`` dB below s; returns float32 (s_hat, s, n)."""
    s = rng.standard_normal(L)
    n = rng.standard_normal(L)
    e = rng.standard_normal(L) * 10.0 ** (-art_db / 20.0)
    return (0.7 * s + g * n + e).astype(dtype), s.astype(dtype), n.astype(dtype)


_DRAWN = {}


def draw(L, k):
    """(s_hat, s, n, ratios, alphas) of length L with the k-th (gain, artefact) pair: float32 signals s_hat = 0.7 s + g n +
    e and their float64 reference, drawn (next seed on a miss, judged by the REFERENCE alone) so that every ratio lies in
    [-10, 60] dB and the condition number of both projections is below 1e3; computed once per (L, k) and shared."""
    if (L, k) not in _DRAWN:
        g, art = GAINS[k % 3], ART_DB[(k // 3) % 3]
        for seed in range(100 * k, 100 * k + 100):
            e, s, n = mix(np.random.default_rng([L, seed]), L, g, art)
            r = np.array(energy_ratios(e, s, n))
            e64, s64, n64 = (x.astype(np.float64) for x in (e, s, n))
            cond = max(np.abs(e64 * s64).sum() / abs(np.dot(e64, s64)), np.abs(e64 * n64).sum() / abs(np.dot(e64, n64)))
            if np.all((r >= -10.0) & (r <= 60.0)) and cond < 1e3:
                break
        else:
            raise AssertionError("no draw of length %d with every ratio in [-10, 60] dB" % L)
        for x in (e, s, n):
            x.setflags(write=False)
        _DRAWN[(L, k)] = (e, s, n, r, np.array(alphas(e, s, n)), seed - 100 * k)
    return _DRAWN[(L, k)][:5]


def draw_misses(L, k):
    """how many seeds ``draw(L, k)`` passed over"""
    draw(L, k)
    return _DRAWN[(L, k)][5]


def many_chunk_lengths(chunk):
    """rows of 8 and 16 chunks (add_ascending<8>: one and two trips of the unrolled body, no remainder), of 9 chunks (body
    + a remainder chunk of one sample) and of 10 and 18 chunks (body + two remainder chunks, the last of 5 and 3 samples)"""
    return [8 * chunk, 8 * chunk + 1, 9 * chunk + 5, 16 * chunk, 17 * chunk + 3]


def mixture_of(s, n):
    """(x, n') for third_mode 2: the float32 mixture x = s + n as a file holds it, and the noise the kernel forms from it,
    float64(x) - float64(s)"""
    x = (s + n).astype(np.float32)
    return x, x.astype(np.float64) - s.astype(np.float64)
