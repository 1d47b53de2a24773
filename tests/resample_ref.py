"""Float64 restatement of the resampler (include/avvad.h, "Rational-rate resampling"), numpy only.

    out[n] = sum_m h[n down + half - m up] x[m],  m over the inputs that exist in
             [ceil((n down - half) / up), floor((n down + half) / up)],  0 <= n < ceil(L up / down)

with scipy.signal.resample_poly's default taps.  Beside every value the absolute-value evaluation A[n] = sum |h| |x| over
the same terms, from which the tests' bound is DERIVED, not measured:

    tol[n] = 2^-24 |ref[n]| + 4 T 2^-53 A[n],   T = 2 half // up + 1 the most terms of an output

The first term is the single rounding to float32.  A double chain of at most T fma's is off by at most T 2^-53 A (first
order); the kernel's chain and this file's dot product each owe that, and the factor 4 leaves room for the higher-order
terms and for the rounding of a value that sits just across a float32 binade from ref.
"""
import math

import numpy as np


def params(up, down):
    """-> (half, T terms per output at most, H floats of stream state per row)"""
    half = 10 * max(up, down)
    return half, 2 * half // up + 1, 2 * half // up + 2


def taps(up, down):
    """up * firwin(2 half + 1, 1 / max(up, down), window=("kaiser", 5.0)), float64"""
    m = max(up, down)
    half = 10 * m
    k = np.arange(2 * half + 1, dtype=np.float64) - half
    h = (1.0 / m) * np.sinc(k * (1.0 / m)) * np.kaiser(2 * half + 1, 5.0)
    return up * (h / h.sum())


def length(L, up, down):
    return -((-L * up) // down)


def emitted(N, up, down):
    """outputs whose every tap has arrived after N inputs"""
    a = N * up - 1 - params(up, down)[0]
    return a // down + 1 if a >= 0 else 0


def outputs(x, pos0, first, last, n0, n1, up, down, h=None):
    """Outputs n0 .. n1 - 1 (absolute) of a row whose input at absolute position pos0 + i is x[i]; the inputs that exist
    are first .. last (absolute), the rest are skipped.  -> (values, A), float64."""
    h = taps(up, down) if h is None else h
    half = params(up, down)[0]
    x = np.asarray(x, dtype=np.float64)
    val, A = np.zeros(max(n1 - n0, 0)), np.zeros(max(n1 - n0, 0))
    for i, n in enumerate(range(n0, n1)):
        lo = max(first, -((half - n * down) // up))
        hi = min(last, (n * down + half) // up)
        if hi < lo:
            continue
        ms = np.arange(lo, hi + 1)
        hh, xx = h[n * down + half - ms * up], x[lo - pos0:hi + 1 - pos0]
        val[i], A[i] = np.dot(hh, xx), np.dot(np.abs(hh), np.abs(xx))
    return val, A


def resample(x, up, down):
    """The whole utterance.  -> (out float64 [ceil(L up / down)], A)"""
    return outputs(x, 0, 0, len(x) - 1, 0, length(len(x), up, down), up, down)


def tol(ref, A, up, down):
    return 2.0 ** -24 * np.abs(ref) + 4 * params(up, down)[1] * 2.0 ** -53 * A


class Stream:
    """The streamed form of one row: ``push(packet, final)`` returns the outputs that call emits (values, A).  Like the
    kernel it carries the last ``hist`` inputs (default H) and nothing else; ``start``: the absolute input position the row
    is preset to, everything before it being zeros.  ``held_max``: the most inputs the next output still needed after a
    call, which H must cover."""

    def __init__(self, up, down, start=0, hist=None):
        self.up, self.down = up, down
        self.half, self.T, self.H = params(up, down)
        self.hist = self.H if hist is None else hist
        self.h = taps(up, down)
        self.total, self.out = start, emitted(start, up, down)
        self.buf = np.zeros(min(self.hist, start))                  # absolute positions total - len(buf) .. total - 1
        self.held_max = 0

    def push(self, packet, final=False):
        packet = np.asarray(packet, dtype=np.float64)
        src = np.concatenate([self.buf, packet])
        pos0 = self.total - len(self.buf)
        self.total += len(packet)
        e = length(self.total, self.up, self.down) if final else emitted(self.total, self.up, self.down)
        e = max(e, self.out)
        res = outputs(src, pos0, pos0, self.total - 1, self.out, e, self.up, self.down, self.h)
        self.out = e
        self.buf = src[max(len(src) - self.hist, 0):]
        first = max(0, -((self.half - e * self.down) // self.up))
        if not final:
            self.held_max = max(self.held_max, self.total - first)
        return res


def stream(x, packets, up, down, start=0, final=True, hist=None):
    """x cut into ``packets`` (sizes; they must sum to len(x)), the last one ``final``.  -> (values, A, Stream)"""
    assert sum(packets) == len(x)
    s, at, vals, As = Stream(up, down, start, hist), 0, [], []
    for i, p in enumerate(packets):
        v, a = s.push(x[at:at + p], final and i == len(packets) - 1)
        at += p
        vals.append(v)
        As.append(a)
    return np.concatenate(vals) if vals else np.zeros(0), np.concatenate(As) if As else np.zeros(0), s
