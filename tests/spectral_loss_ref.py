"""Float64 restatement of the mask-regression losses (csrc/spectral_loss.hip, ``ops.spectral_loss``), the shared case
list, a float32 stand-in, the assertions every implementation goes through (``check_spectral``) and the mistakes those
assertions must reject.  A plain module: torch on the CPU only.

With the mask m = pred (pred_mode 1) or sigmoid(pred) (pred_mode 2), per cell (b, t, f)
    "mask"      (y - m)^2
    "signal"    ((y - m) x)^2, x = |X|
    "spectrum"  |S - m X|^2 as a complex difference, real(d conj(d))
row_b = (1 / len_b) sum_{t < len_b} sum_f term, loss = sum_b row_b, len_b clamped to [0, T]; a row of length 0 adds
nothing.  The gradient comes from autograd in double.

Bounds.  They are not chosen: ``standin`` evaluates the same formula in float32 (terms and analytic gradients in float32,
every sum in float64, the loss rounded to float32 as the kernel stores it), and its error against float64 is measured
over every (case, kind, pred_mode) of the list -- relative for ``loss`` and ``row_loss``, and for ``dpred`` relative to
the row's largest gradient magnitude.  The bound of a quantity is 8 times the largest such error, the margin the
streaming and encoder oracles keep over their stand-ins.  Measured (``measure_standin()``):
    loss      1.44e-07      ("one", signal, pred_mode 1: a single float32 term; 2^-23 = 1.19e-07)
    row_loss  1.44e-07      (the same case)
    dpred     5.64e-07      ("ragged", mask, pred_mode 2: float32 sigmoid, then the cancellation in 1 - m)
The two shapes that turn the finishing loops, "chunks130" (rows of 130, 65, 64 and 0 chunks) and "rows67" (B = 67), were
added under these bounds as they stood; the stand-in's largest errors on them are
    chunks130   loss 4.37e-08   row_loss 2.05e-09   dpred 5.62e-07   (mask, pred_mode 2, as "ragged")
    rows67      loss 2.49e-08   row_loss 8.85e-08   dpred 1.08e-06   (signal, pred_mode 2, row 4)
all below the bounds, and the list's worst dpred error is now the 1.08e-06 of "rows67": its row 4 has one frame, whose
largest gradient is 0.78, and a logit of 5.08 in it, where m = 0.9938 and float32 leaves 1 - m with a relative error of
2^-24 / 0.0062 = 9.6e-06 on a gradient of 0.097.  Any float32 evaluation of m (1 - m) carries that, so BOUND_DPRED stands
4.2 times over the stand-in here -- still inside the window of 4 to 16 times that tests/test_spectral_loss_cpu.py keeps
between a bound and the stand-in's worst error.  The loops these two shapes turn add partials and rows; none touches dpred.
"""
import functools
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = int(re.search(r"#define AVVAD_SPECTRAL_CHUNK (\d+)", open(os.path.join(ROOT, "include", "avvad.h")).read()).group(1))

KINDS = ("mask", "signal", "spectrum")
MODES = (1, 2)
BOUND_LOSS = 8 * 1.44e-07
BOUND_ROWS = 8 * 1.44e-07
BOUND_DPRED = 8 * 5.64e-07

# name -> (B, T, F, lengths or None).  T and F are odd wherever they can be, so that no row of [T][F] floats starts on 16
# bytes; "boundary": F = 1 puts len * F one cell below, on and one cell above the chunk; "three": one row over three chunks;
# "clamped": lengths outside [0, T]; "saturated" (pred_mode 2 only): logits of +-30 and +-100 among ordinary ones.
# The last two turn the loops of spectral_finish (and reach workgroups with blockIdx.x >= 64 in spectral_pass):
# "chunks130": rows of 130, 65, 64 and 0 chunks -- three trips of a wave's lane loop over a row's partials, two trips whose
# second holds one chunk, exactly one full trip, an empty row; "rows67": B = 67 -- five trips of the wave-per-row loop
# (16 waves) and two of the final sum over rows (64 lanes), rows 64 to 66 of lengths 5, 3 and 7.
T3 = 2 * CHUNK // 513 + 1 + (2 * CHUNK // 513) % 2          # odd, and T3 * 513 lies in (2 CHUNK, 3 CHUNK]
SHAPES = {
    "one": (1, 1, 1, None),
    "small": (2, 3, 5, None),
    "ragged": (3, 7, 513, (7, 4, 0)),
    "boundary": (3, CHUNK + 3, 1, (CHUNK - 1, CHUNK, CHUNK + 1)),
    "three": (1, T3, 513, None),
    "clamped": (2, 3, 5, (9, -2)),
    "saturated": (2, 5, 7, (5, 3)),
    "batch5": (5, 7, 33, (7, 5, 3, 7, 1)),
    "chunks130": (4, 517, 513, (517, 257, 255, 0)),
    "rows67": (67, 7, 33, tuple([7, 5, 3, 7, 1, 0, 6][b % 7] for b in range(67))),
}
CASES = [(n, k, m) for n in SHAPES for k in KINDS for m in MODES if not (n == "saturated" and m == 1)]


def n_chunks(T, F):
    return -(-T * F // CHUNK)


@functools.lru_cache(maxsize=None)
def case(name, kind, pred_mode):
    """The inputs of one case as float32 / complex64 CPU tensors (built once, never changed): pred (B, T, F) -- mask
    probabilities in (0, 1) for pred_mode 1, logits for 2 --, target in [0, 1], mix X and speech S = y X + a little."""
    B, T, F, lengths = SHAPES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 7 + 1)
    if pred_mode == 1:
        pred = torch.rand(B, T, F, generator=g) * 0.98 + 0.01
    else:
        pred = torch.randn(B, T, F, generator=g) * 3.0
        if name == "saturated":
            flat = pred.view(B, -1)
            flat[:, 1], flat[:, 4], flat[:, 8], flat[:, 11] = 30.0, -30.0, 100.0, -100.0
    target = torch.rand(B, T, F, generator=g)
    mix = torch.complex(torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g))
    speech = target * mix + 0.1 * torch.complex(torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g))
    return {"name": name, "kind": kind, "pred_mode": pred_mode, "B": B, "T": T, "F": F, "lengths": lengths, "pred": pred,
            "target": target, "mix": mix, "speech": speech}


def single_row(c, b):
    """row b of a case as a case of its own (B = 1)"""
    one = dict(c)
    one.update(B=1, lengths=None if c["lengths"] is None else (c["lengths"][b],), name="%s[%d]" % (c["name"], b))
    for k in ("pred", "target", "mix", "speech"):
        one[k] = c[k][b:b + 1]
    return one


def lens_of(c):
    if c["lengths"] is None:
        return [c["T"]] * c["B"]
    return [min(max(int(n), 0), c["T"]) for n in c["lengths"]]


def terms(kind, m, y, X, S):
    """the reference's three formulas as they stand, per cell"""
    if kind == "mask":
        return torch.square(y - m)
    if kind == "signal":
        return torch.square(torch.mul(y - m, X.abs()))
    d = S - m * X
    return torch.real(d * d.conj())


def _reference(c):
    p = c["pred"].to(torch.float64).requires_grad_(True)
    m = torch.sigmoid(p) if c["pred_mode"] == 2 else p
    t = terms(c["kind"], m, c["target"].to(torch.float64), c["mix"].to(torch.complex128), c["speech"].to(torch.complex128)).sum(-1)
    rows = [t[b, :n].sum() / n if n > 0 else t.new_zeros(()) for b, n in enumerate(lens_of(c))]
    loss = torch.stack(rows).sum()
    loss.backward()
    return float(loss.detach()), torch.stack(rows).detach().numpy().copy(), p.grad.numpy().copy()


_REF = {}


def reference(c):
    """(loss, rows (B,), dpred (B, T, F)) in float64; computed once per case and shared"""
    key = (c["name"], c["kind"], c["pred_mode"])
    if key not in _REF:
        _REF[key] = _reference(c)
    return _REF[key]


LOOP_MUTANTS = {                # name -> (shape, kind, pred_mode) of the case that shows it; no earlier shape can
    "finish_first_64_chunks": ("chunks130", "spectrum", 2),   # a row's sum takes only cells below 64 * CHUNK of its flat run
    "finish_first_16_rows": ("rows67", "spectrum", 2),        # rows b >= 16 get row loss 0 and add nothing
    "loss_first_64_rows": ("rows67", "spectrum", 2),          # rows are right, the loss adds rows[:64]
}

MUTANTS = {                     # name -> (kind, pred_mode) of the "ragged" case that shows it
    "divide_by_T": ("mask", 2),
    "padded_gradient": ("signal", 1),
    "magnitude_difference": ("spectrum", 1),
    "no_sigmoid_factor": ("mask", 2),
    "x_squared": ("signal", 2),
    "mean_over_F": ("spectrum", 2),
    "empty_row_nan": ("mask", 1),
}


def standin(c, mutant=None):
    """The same formula in float32 with analytic gradients, float64 sums and a float32 loss; ``mutant``: one of MUTANTS
    or LOOP_MUTANTS."""
    B, T, F = c["B"], c["T"], c["F"]
    p, y = c["pred"], c["target"]
    X, S = c["mix"], c["speech"]
    m = torch.sigmoid(p) if c["pred_mode"] == 2 else p
    if c["kind"] == "mask":
        d = y - m
        term, g = d * d, -2.0 * d
    elif c["kind"] == "signal":
        x = torch.sqrt(X.real * X.real + X.imag * X.imag)
        if mutant == "x_squared":
            x = x * x
        d = (y - m) * x
        term, g = d * d, -2.0 * d * x
    elif mutant == "magnitude_difference":
        d = S.abs() - m * X.abs()
        term, g = d * d, -2.0 * d * X.abs()
    else:
        dr, di = S.real - m * X.real, S.imag - m * X.imag
        term, g = dr * dr + di * di, -2.0 * (dr * X.real + di * X.imag)
    if c["pred_mode"] == 2 and mutant != "no_sigmoid_factor":
        g = g * (m * (1.0 - m))
    assert term.dtype == g.dtype == torch.float32
    rows = np.zeros(B, dtype=np.float64)
    dpred = np.zeros((B, T, F), dtype=np.float32)
    for b, n in enumerate(lens_of(c)):
        div = T if mutant == "divide_by_T" else n
        if n > 0 or mutant == "empty_row_nan":
            with np.errstate(all="ignore"):
                run = term[b, :n].reshape(-1)[:64 * CHUNK] if mutant == "finish_first_64_chunks" else term[b, :n]
                rows[b] = np.float64(run.to(torch.float64).sum().item()) / np.float64(div)
        if mutant == "mean_over_F":
            rows[b] /= F
        if n > 0:
            cut = T if mutant == "padded_gradient" else n
            scale = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(div), dtype=torch.float32)
            dpred[b, :cut] = (g[b, :cut] * scale).numpy() / (F if mutant == "mean_over_F" else 1)
    if mutant == "finish_first_16_rows":
        rows[16:] = 0.0
    return float(np.float32(rows[:64].sum() if mutant == "loss_first_64_rows" else rows.sum())), rows, dpred


def errors(got, c):
    """(loss, rows, dpred) errors of ``got`` against float64 as the bounds measure them; structural mistakes -- a wrong
    shape, a non-finite value, anything but zeros on an empty row or on padded frames -- are AssertionErrors."""
    loss, rows, dpred = got
    ref_loss, ref_rows, ref_d = reference(c)
    rows, dpred = np.asarray(rows, dtype=np.float64), np.asarray(dpred)
    what = "%s %s pred_mode %d" % (c["name"], c["kind"], c["pred_mode"])
    assert rows.shape == ref_rows.shape and dpred.shape == ref_d.shape and dpred.dtype == np.float32, what
    assert np.isfinite(loss) and np.isfinite(rows).all() and np.isfinite(dpred).all(), "%s: a value is not finite" % what
    e_loss = abs(loss - ref_loss) / abs(ref_loss) if ref_loss != 0.0 else abs(loss)
    e_rows = e_d = 0.0
    for b, n in enumerate(lens_of(c)):
        assert not dpred[b, n:].any(), "%s: row %d has a gradient on padded frames" % (what, b)
        if n == 0:
            assert rows[b] == 0.0, "%s: the empty row %d has the loss %r" % (what, b, rows[b])
            continue
        e_rows = max(e_rows, abs(rows[b] - ref_rows[b]) / abs(ref_rows[b]))
        e_d = max(e_d, float(np.abs(dpred[b].astype(np.float64) - ref_d[b]).max() / np.abs(ref_d[b]).max()))
    return e_loss, e_rows, e_d


def check_spectral(fn, c):
    """``fn(case)`` -> (loss as a Python float, rows (B,) float64, dpred (B, T, F) float32 numpy) within the bounds"""
    got = fn(c)
    e_loss, e_rows, e_d = errors(got, c)
    what = "%s %s pred_mode %d" % (c["name"], c["kind"], c["pred_mode"])
    print("%-28s loss %.3e (<= %.3e)  rows %.3e (<= %.3e)  dpred %.3e (<= %.3e)"
          % (what, e_loss, BOUND_LOSS, e_rows, BOUND_ROWS, e_d, BOUND_DPRED))
    assert e_loss <= BOUND_LOSS, "%s: loss off by %.3e relative (bound %.3e)" % (what, e_loss, BOUND_LOSS)
    assert e_rows <= BOUND_ROWS, "%s: row_loss off by %.3e relative (bound %.3e)" % (what, e_rows, BOUND_ROWS)
    assert e_d <= BOUND_DPRED, "%s: dpred off by %.3e of the row's largest gradient (bound %.3e)" % (what, e_d, BOUND_DPRED)
    return got


def measure_standin():
    """the largest stand-in error per quantity over the case list: what the bounds above are 8 times of"""
    worst = np.zeros(3)
    for key in CASES:
        c = case(*key)
        worst = np.maximum(worst, errors(standin(c), c))
    return tuple(worst)


if __name__ == "__main__":
    print("stand-in: loss %.3e  rows %.3e  dpred %.3e" % measure_standin())
