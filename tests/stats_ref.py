"""Float64 restatement of the train-set standardisation statistics (the reference's scripts/create_audio_train_files.py:
196-214, 340-392): per-bin n, sum and sum of squares of the log-power spectrogram over every frame of the set,
``mean = sum / n``, ``std = sqrt((sumsq - n mean^2) / (n - 1))`` -- plus the reference's literal float32 accumulation, for
the CPU comparison of the two.  Exact integer-valued batches, the chunk / segment arithmetic of csrc/stats.hip restated, a
host model of its kernels with planted mistakes, and the bound on two orders of a double sum.  Test infrastructure only."""
import math
import os

import numpy as np

from conftest import GOLDEN

N_FFT, HOP, FS, EPS = 1024, 256, 16e3, 1e-8


def utterances():
    """The three fixture utterances as float32 waveforms (int16 / 32768, not yet peak-normalised): noisy sa1, clean sa1 and
    the first 30000 samples of the noisy one -- 185 + 185 + 115 = 485 frames, three lengths, so every batch is ragged."""
    noisy = np.load(os.path.join(GOLDEN, "utt_sa1.npz"))["samples"].astype(np.float32) / 32768.0
    clean = np.load(os.path.join(GOLDEN, "utt_sa1_clean.npz"))["samples"].astype(np.float32) / 32768.0
    return [noisy, clean, noisy[:30000].copy()]


def end_padded(x):
    """stft_pytorch's end pad (packages/processing/stft.py:134-139), the rule of ``ops.n_frames``."""
    v = len(x) / FS / (N_FFT / FS) / (HOP / N_FFT)
    return np.pad(x, (0, HOP)) if math.ceil(v) != int(v) else x


def features64(x, normalise=True):
    """(513, T) float64 log-power features of one utterance: x / max|x|, end pad, framed float64 DFT, log(|S|^2 + eps)."""
    from oracle import frontend
    x = np.asarray(x, dtype=np.float64)
    if normalise:
        x = x / np.max(np.abs(x))
    S = frontend.stft_naive(end_padded(x), N_FFT, HOP)
    return np.log(S.real ** 2 + S.imag ** 2 + EPS)


def accumulate(feats, dtype=np.float64):
    """[sum (F), sumsq (F), count] over a list of (F, T_i) feature arrays, the accumulator layout of ``ops.stats_new``."""
    F = feats[0].shape[0]
    acc = np.zeros(2 * F + 1, dtype)
    for x in feats:
        x = x.astype(dtype)
        acc[:F] += x.sum(axis=-1)
        acc[F:2 * F] += (x ** 2).sum(axis=-1)
        acc[2 * F] += x.shape[-1]
    return acc


def finalize(acc):
    """(mean, std) by the reference's formula, in the accumulator's precision."""
    F = (len(acc) - 1) // 2
    n = acc[2 * F]
    mean = acc[:F] / n
    std = np.sqrt((1 / (n - 1)) * (acc[F:2 * F] - n * mean ** 2))
    return mean, std


def stats64(feats):
    return finalize(accumulate(feats))


# ------------------------------------------------------------------------------------------ exact operands
# Integer-valued float32 inputs with |x| <= 2^10: every sum and sum of squares below is an integer under 2^53, exact in
# double in any order, so a correct accumulator equals the host's integers bit for bit and a dropped or doubled partial,
# row or column is a mismatch, never a rounding question.
ROWS_PER_CHUNK, SCALAR_CHUNK_ELEMS, ADD_WAVES, ADD_UNROLL, UN = 128, 16384, 16, 8, 8     # csrc/stats.hip


def exact_batch(B, T, F, seed):
    """(B, T, F) float32 of integers in -1024..1024"""
    rng = np.random.default_rng(seed)
    return rng.integers(-1024, 1025, size=(B, T, F)).astype(np.float32)


def ragged_lengths(B, T, seed):
    """B lengths that include 0, T, T + 7 (above the batch) and -2 (below zero) wherever B allows, the rest in 0..T"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, T + 1, size=B)
    for i, v in zip(rng.permutation(B)[:4], (T + 7, -2, 0, T)):
        lens[i] = v
    return [int(v) for v in lens]


def clamp(lengths, B, T):
    return [T] * B if lengths is None else [min(max(int(n), 0), T) for n in lengths]


def host_sums(x, lengths, nstat):
    """float64 [sum (nstat), sumsq (nstat), count] of the rows t < min(max(lengths[b], 0), T): the accumulator a call of
    ``ops.accumulate_stats`` adds (count in values for nstat == 1 != F, in rows otherwise)"""
    x = np.asarray(x, np.float64)
    B, T, F = x.shape
    rows = np.concatenate([x[b, :n] for b, n in enumerate(clamp(lengths, B, T))]).reshape(-1, F)
    if nstat == F:
        return np.concatenate([rows.sum(axis=0), (rows * rows).sum(axis=0), [float(rows.shape[0])]])
    return np.array([rows.sum(), (rows * rows).sum(), float(rows.size)])


def n_chunks(rows, F, nstat):
    """chunks of one call: 128 rows in the per-column form (also nstat == F == 1), 16384 // F rows (at least one) in the
    scalar form"""
    per = ROWS_PER_CHUNK if (nstat != 1 or F == 1) else (1 if F >= SCALAR_CHUNK_ELEMS else SCALAR_CHUNK_ELEMS // F)
    return -(-rows // per), per


def segments(nchunks):
    """add_partials: (k0, k1) of the sixteen waves and ``per``"""
    per = -(-nchunks // ADD_WAVES)
    return [(w * per, max(w * per, min(nchunks, w * per + per))) for w in range(ADD_WAVES)], per


def branches(B, T, F, nstat, lengths=None):
    """which paths of csrc/stats.hip a call takes, from the shape alone"""
    rows = B * T
    nchunks, rows_per = n_chunks(rows, F, nstat)
    segs, per = segments(nchunks)
    column = nstat == F
    out = dict(form="column" if column else "scalar", nchunks=nchunks, rows_per_chunk=rows_per, per=per,
               unrolled=[(k1 - k0) // ADD_UNROLL for k0, k1 in segs], remainder=[(k1 - k0) % ADD_UNROLL for k0, k1 in segs],
               ragged_last_chunk=rows % rows_per, count_trips=-(-B // (64 * ADD_WAVES)) if lengths is not None else 0)
    if column:
        out.update(col_blocks=-(-F // 64), lanes_in_last_block=F - 64 * (-(-F // 64) - 1),
                   boundaries_per_group=(UN - 1) // T + 1 if lengths is not None else 0)
    else:
        out.update(row_trips=-(-F // 256), idle_lanes=max(0, 256 - F))
    return out


def column_walk(x2, T, lengths, m0, m1, reset_t=True):
    """One wave of column_partials on rows m0..m1 of x2 (rows, F): (b, t, len) advance with the rows, eight rows per group;
    returns (sum, sumsq) per column.  MUTANT ``reset_t=False``: t is not set back to 0 at an utterance boundary."""
    F = x2.shape[1]
    s, q = np.zeros(F), np.zeros(F)
    ragged = lengths is not None
    b = m0 // T if ragged else 0
    t = m0 - b * T if ragged else 0
    ln = lengths[b] if (ragged and m0 < m1) else 0
    for m in range(m0, m1, UN):
        for u in range(UN):
            on = m + u < m1 and (not ragged or t < ln)
            if ragged:
                t += 1
                if t == T:
                    if reset_t:
                        t = 0
                    b += 1
                    if m + u + 1 < m1:
                        ln = lengths[b]
            if on:
                s += x2[m + u]
                q += x2[m + u] * x2[m + u]
    return s, q


def model_accumulate(x, lengths, nstat, mutant=None):
    """The kernels' arithmetic restated on the host (float64, exact on ``exact_batch``): chunk partials (four waves of 32
    rows walking (b, t, len) in the per-column form, whole rows in the scalar form), sixteen segments of chunks added with
    an eight-way body and a remainder loop, the clamped count.  ``mutant`` plants one mistake: "no_unroll" (the eight-way
    body adds nothing), "drop_last_segment", "no_clamp" (count = sum of the raw lengths), "no_t_reset"."""
    x = np.asarray(x, np.float64)
    B, T, F = x.shape
    x2 = x.reshape(B * T, F)
    rows = B * T
    nchunks, rows_per = n_chunks(rows, F, nstat)
    part = np.zeros((nchunks, 2 * nstat))
    for c in range(nchunks):
        c0, c1 = c * rows_per, min(rows, (c + 1) * rows_per)
        if nstat == F:
            for wv in range(4):
                m0 = c0 + wv * (ROWS_PER_CHUNK // 4)
                s, q = column_walk(x2, T, lengths, m0, min(rows, m0 + ROWS_PER_CHUNK // 4), reset_t=mutant != "no_t_reset")
                part[c, :F] += s
                part[c, F:] += q
        else:
            for m in range(c0, c1):
                if lengths is None or m - (m // T) * T < lengths[m // T]:
                    part[c, 0] += x2[m].sum()
                    part[c, 1] += (x2[m] * x2[m]).sum()
    acc = np.zeros(2 * nstat + 1)
    segs, _ = segments(nchunks)
    for w, (k0, k1) in enumerate(segs):
        if mutant == "drop_last_segment" and w == max(i for i, (a, b) in enumerate(segs) if b > a):
            continue
        k = k0
        while k + ADD_UNROLL <= k1:
            if mutant != "no_unroll":
                acc[:-1] += part[k:k + ADD_UNROLL].sum(axis=0)
            k += ADD_UNROLL
        acc[:-1] += part[k:k1].sum(axis=0)
    count = sum(lengths) if (mutant == "no_clamp" and lengths is not None) else sum(clamp(lengths, B, T))
    acc[-1] = count * (1.0 if nstat == F else float(F))
    return acc


# (name, B, T, F, nstat, ragged): the shapes of test_stats_gpu.py's exact cases, each the smallest that reaches the branch
# it is named for (tests/test_stats_cpu.py checks that it does)
EXACT_CASES = [
    ("one column, column form", 40, 1, 1, 1, True),              # nstat == F == 1 takes column_partials; T = 1: 8 boundaries / group
    ("F 63: idle lane", 37, 3, 63, 63, True),                    # F < 64; T = 3: three boundaries per group
    ("F 64: one full block", 29, 5, 64, 64, True),               # T = 5: two boundaries per group
    ("F 65: one lane in block 2", 9, 33, 65, 65, True),          # F = 64 k + 1; T = 33 > one wave's 32 rows
    ("F 129: one lane in block 3", 50, 5, 129, 129, True),
    ("F 65 whole batch", 9, 33, 65, 65, False),
    ("150 chunks + 37 rows", 128 * 150 + 37, 1, 65, 65, True),   # add_partials' eight-way body and remainder, count loop x 19
    ("scalar F 2", 6, 3, 2, 1, True),                            # F < 256: lanes sit idle
    ("scalar F 200", 6, 3, 200, 1, True),
    ("scalar F 5000", 6, 3, 5000, 1, True),
    ("scalar F 16383", 6, 3, 16383, 1, True),                    # the last F with 16384 // F rows per chunk
    ("scalar F 16384", 6, 3, 16384, 1, True),                    # one row per chunk from here on
    ("scalar F 20000", 6, 3, 20000, 1, True),
    ("scalar count loop", 1030, 1, 7, 1, True),                  # B > 1024: second trip of the count loop
]


def exact_case(name):
    """(x (B, T, F) float32, lengths or None, nstat) of one of EXACT_CASES"""
    i = [c[0] for c in EXACT_CASES].index(name)
    _, B, T, F, nstat, ragged = EXACT_CASES[i]
    return exact_batch(B, T, F, seed=100 + i), (ragged_lengths(B, T, seed=200 + i) if ragged else None), nstat


def sum_bound(values, n):
    """|double sum in one order - double sum in another| of n terms: each side errs by at most (n - 1) 2^-53 sum|x_i|
    (every partial sum is bounded by sum|x_i|), so two sides differ by at most 2 (n - 1) 2^-53 sum|x_i|."""
    return 2.0 * max(n - 1, 0) * 2.0 ** -53 * np.abs(values).sum(axis=0)


def stats32_literal(feats):
    """The reference as written: float32 spectrograms, ``n_samples, channels_sum, channels_squared_sum = 0., 0., 0.`` then
    ``+=`` of every file's float32 ``np.sum`` (a Python float plus a float32 array stays float32), float32 division."""
    n_samples, channels_sum, channels_squared_sum = 0., 0., 0.
    for x in feats:
        x = x.astype(np.float32)
        n_samples += x.shape[-1]
        channels_sum += np.sum(x, axis=-1)
        channels_squared_sum += np.sum(x ** 2, axis=-1)
    assert channels_sum.dtype == np.float32
    mean = channels_sum / n_samples
    std = np.sqrt((1 / (n_samples - 1)) * (channels_squared_sum - n_samples * mean ** 2))
    return mean, std
