"""A float64 numpy restatement of the STREAMED overlap-add of csrc/istft_stream.hip: frames come in a few at a time, the
samples no later frame can cover go out, and each row's unfinished sums travel in a ``(n_fft,)`` state.  It states the
recurrence the kernel implements, so that the CPU tests can prove it against ``istft_ref.istft64`` (the whole-utterance
oracle) for every split of a stream; the GPU tests use it to drive the same schedules.

``step`` mirrors the kernel's contract: row with ``e0`` frames behind it, ``nf`` frames in the call, ``n_out`` samples to
emit.  Output ``p`` is the absolute sample ``e0 hop + p``; it starts from ``state[p]`` (0 for ``p >= n_fft``) and adds
``Y[i][p - i hop]`` in ascending ``i``.  The new state is the partial sum of the samples from ``(e0 + nf) hop`` on; a row
whose ``n_out`` differs from ``nf hop`` ends with the call, and its state is all zero."""
import numpy as np

import istft_ref as R


def frame_inverses(S, n_fft):
    """S complex (T, F) -> Y (T, n_fft) float64: hann * irfft of every frame (what the product kernel computes)"""
    S = np.asarray(S, dtype=np.complex128).reshape(-1, n_fft // 2 + 1)
    return R.hann(n_fft)[None, :] * np.fft.irfft(S, n=n_fft, axis=1) if S.shape[0] else np.zeros((0, n_fft))


def step(Y, state, e0, n_out, n_fft, hop):
    """-> (num (n_out,), wss (n_out,), new state (n_fft,)): the numerators and window sums of squares of the samples
    emitted, before the division."""
    nf = Y.shape[0]
    span = max(n_out, nf * hop + n_fft, n_fft)
    acc = np.zeros(span)
    acc[:n_fft] = state
    for i in range(nf):                                   # ascending: the whole-utterance chain, cut at the call boundary
        acc[i * hop:i * hop + n_fft] += Y[i]
    w2 = R.hann(n_fft) ** 2
    wss = np.zeros(n_out)
    for p in range(n_out):
        s = e0 * hop + p
        t0 = max(0, -((n_fft - 1 - s) // hop))            # ceil((s - n_fft + 1) / hop)
        for t in range(t0, min(s // hop, e0 + nf - 1) + 1):
            wss[p] += w2[s - t * hop]
    if nf == 0 and n_out == 0:
        new = state.copy()
    elif n_out != nf * hop:
        new = np.zeros(n_fft)
    else:
        new = acc[nf * hop:nf * hop + n_fft].copy()
    return acc[:n_out].copy(), wss, new


def stream(S, calls, n_fft, hop):
    """One row: S complex (T, F), ``calls`` a list of (frames, n_before, n_out) as ``OlaClock.advance`` hands them out
    -> (y, num, wss) float64 over all emitted samples, and the last state."""
    Y = frame_inverses(S, n_fft)
    state = np.zeros(n_fft)
    nums, wsss, t = [], [], 0
    for nf, e0, n_out in calls:
        assert e0 == t
        num, wss, state = step(Y[t:t + nf], state, e0, n_out, n_fft, hop)
        nums.append(num)
        wsss.append(wss)
        t += nf
    assert t == Y.shape[0]
    num, wss = np.concatenate(nums), np.concatenate(wsss)
    y = num.copy()
    nz = wss > R.TINY32
    y[nz] /= wss[nz]
    return y, num, wss, state
