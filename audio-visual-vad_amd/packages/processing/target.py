"""Drop-in for ``packages/processing/target.py`` (``clean_speech_VAD :5-56``, ``clean_speech_IBM :58-70``,
``noise_robust_clean_speech_IBM :72-107``) with the reference's signatures and defaults, computed by the HIP label
kernels (``csrc/target.hip``).

A GPU tensor in gives a GPU tensor out.  A numpy array or a CPU tensor -- what the reference's scripts pass -- is moved
to the current GPU, labelled there and returned as a float32 numpy array in the reference's shape: ``(1, T)`` for the
VAD, ``(F, T)`` for the masks.  This is not a CPU fallback: without a GPU every function raises ``AvvadError``, like
``stft_pytorch``.  ``pad_mode`` may be ``'reflect'`` or ``'constant'``.

``noise_aware_IBM`` and ``threshold_IBM`` (``:151-251``) take spectra of shape (frames, bins), complex, as the reference
does, and return boolean masks of that shape: GPU tensors for GPU tensors, numpy arrays for host input.  Spectra are read
as complex64."""
import numpy as np
import torch


def _on_gpu(x, what):
    """-> (float32 tensor on the GPU, came from the host?)"""
    from avvad._lib import AvvadError
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x, False
    if not torch.cuda.is_available():
        raise AvvadError("%s: the label kernels run on the GPU and none is present -- there is no CPU fallback" % what)
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to("cuda"), True


def _vad(speech_t, fs, wlen_sec, hop_percent, center, pad_mode, pad_at_end, vad_threshold):
    from avvad import ops
    x, host = _on_gpu(speech_t, "clean_speech_VAD")
    x = x.reshape(-1).float().contiguous()
    _, vad = ops.speech_targets(x.view(1, -1), [x.numel()], "vad_labels", fs=fs, wlen_sec=wlen_sec, hop_percent=hop_percent,
                                center=center, pad_mode=pad_mode, pad_at_end=pad_at_end, vad_threshold=vad_threshold)
    return vad.view(1, -1), host


def _spectrum(speech_tf):
    x, host = _on_gpu(speech_tf, "clean_speech_IBM")
    if x.is_complex():
        x = x.to(torch.complex64)
    else:
        x = x.float()
    return x, host


def clean_speech_VAD(speech_t, fs=16e3, wlen_sec=50e-3, hop_percent=0.25, center=True, pad_mode='reflect', pad_at_end=True,
                     vad_threshold=1.70):
    """Frame energies ``sum(y^2)`` > ``10**vad_threshold * min`` over the utterance -> float32 (1, T)."""
    vad, host = _vad(speech_t, fs, wlen_sec, hop_percent, center, pad_mode, pad_at_end, vad_threshold)
    return vad.cpu().numpy() if host else vad


def clean_speech_IBM(speech_tf, eps=1e-8, ibm_threshold=50):
    """``20 log10(|S| + eps) > max(20 log10(|S| + eps)) - ibm_threshold`` over the whole (F, T) spectrum -> float32 (F, T).
    ``speech_tf``: complex (F, T), or the (F, T, 2) real view ``stft_pytorch`` returns."""
    from avvad import ops
    x, host = _spectrum(speech_tf)
    out = ops.ibm_from_spectrum(x, eps=eps, ibm_threshold=ibm_threshold)
    return out.cpu().numpy() if host else out


def noise_robust_clean_speech_IBM(speech_t, speech_tf, fs=16e3, wlen_sec=50e-3, hop_percent=0.25, center=True, pad_mode='reflect',
                                  pad_at_end=True, vad_threshold=1.70, eps=1e-8, ibm_threshold=50):
    """``clean_speech_IBM(speech_tf) * clean_speech_VAD(speech_t)``, the VAD broadcast over frequency; the two frame counts
    must agree (or the VAD hold one frame), as numpy broadcasting requires."""
    from avvad import ops
    x, host_tf = _spectrum(speech_tf)
    vad, host_t = _vad(speech_t, fs, wlen_sec, hop_percent, center, pad_mode, pad_at_end, vad_threshold)
    T = x.shape[1]
    if vad.shape[1] != T:
        if vad.shape[1] != 1:
            raise ValueError("operands could not be broadcast together: IBM (%d, %d) and VAD %s"
                             % (x.shape[0], T, tuple(vad.shape)))
        vad = vad.expand(1, T).contiguous()
    out = ops.ibm_from_spectrum(x, eps=eps, ibm_threshold=ibm_threshold, vad=vad)
    return out.cpu().numpy() if (host_tf or host_t) else out


def _frames_by_bins(S, what):
    """(frames, bins) complex spectrum -> (complex64 tensor on the GPU, came from the host?)"""
    x, host = _on_gpu(S, what)
    if not x.is_complex() or x.dim() != 2:
        raise ValueError("%s: a complex spectrum of shape (frames, frequency-bins), got %s %s" % (what, x.dtype, tuple(x.shape)))
    return x.to(torch.complex64), host


def noise_aware_IBM(X, N, threshold_unvoiced_speech=5, threshold_voiced_speech=0, threshold_unvoiced_noise=-10,
                    threshold_voiced_noise=-10, low_cut=5, high_cut=500):
    """(speech mask, noise mask) of a speech spectrum ``X`` and a noise spectrum ``N``, both (frames, bins): the speech
    power over a per-bin threshold against the noise power and against 0.005, bins below ``low_cut - 1`` and from
    ``high_cut`` on forced to 0 in the speech mask and to 1 in the noise mask."""
    from avvad import ops
    x, host_x = _frames_by_bins(X, "noise_aware_IBM")
    n, host_n = _frames_by_bins(N, "noise_aware_IBM")
    out = ops.noise_aware_from_spectrum(x, n, outputs=("speech", "noise"), threshold_unvoiced_speech=threshold_unvoiced_speech,
                                        threshold_voiced_speech=threshold_voiced_speech,
                                        threshold_unvoiced_noise=threshold_unvoiced_noise,
                                        threshold_voiced_noise=threshold_voiced_noise, low_cut=low_cut, high_cut=high_cut)
    speech, noise = out["speech"] != 0, out["noise"] != 0
    return (speech.cpu().numpy(), noise.cpu().numpy()) if (host_x or host_n) else (speech, noise)


def threshold_IBM(X, threshold_unvoiced_speech=5, threshold_voiced_speech=0, threshold_unvoiced_noise=-10,
                  threshold_voiced_noise=-10, low_cut=5, high_cut=500):
    """The speech mask of ``noise_aware_IBM`` against a constant noise power of 10 in every cell."""
    from avvad import ops
    x, host = _frames_by_bins(X, "threshold_IBM")
    out = ops.noise_aware_from_spectrum(x, None, outputs=("speech",), threshold_unvoiced_speech=threshold_unvoiced_speech,
                                        threshold_voiced_speech=threshold_voiced_speech,
                                        threshold_unvoiced_noise=threshold_unvoiced_noise,
                                        threshold_voiced_noise=threshold_voiced_noise, low_cut=low_cut, high_cut=high_cut)
    speech = out["speech"] != 0
    return speech.cpu().numpy() if host else speech
