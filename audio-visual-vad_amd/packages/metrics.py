"""Drop-in for the reporting helpers of ``packages/metrics.py`` that the classifier pipeline uses
(``mean_confidence_interval`` ``:5-10``, ``compute_stats`` ``:62-130``; called from
``scripts/run_metrics_dnn_classif.py:292-300``).  Host-side reporting: Student-t confidence half-width of
the per-utterance scores, overall and per input SNR / noise type / speaker, printed as the reference's
``METRIC / AVERAGE / CONF. INT.`` tables (and returned, which the reference does not do).

The speech-enhancement metrics of that file, ``si_sdr_components`` (``:12-37``) and ``energy_ratios`` (``:39-60``),
run on the GPU: one pass over the three signals sums six inner products in double (``avvad.ops.energy_ratios``,
csrc/scores.hip) and the ratios and the two ``alpha`` follow in closed form.  Signatures are the reference's; numpy
arrays in give numpy arrays / floats out, tensors in give tensors out.  The kernel reads float32 samples (what a wav
file holds); float64 input is rounded to float32 first."""
import numpy as np
import scipy.stats


def _on_gpu(*signals):
    """the 1-D signals as float32 GPU tensors (on the device of the first tensor among them, else the current one)"""
    import torch
    dev = next((x.device for x in signals if isinstance(x, torch.Tensor) and x.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    out = []
    for x in signals:
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        out.append(t.detach().to(device=dev, dtype=torch.float32).reshape(-1))
    return out


def si_sdr_components(s_hat, s, n):
    """``s_hat = alpha_s s + alpha_n n + e_art`` -> (s_target, e_noise, e_art): the two projections' coefficients come
    from the GPU's inner products, the three planes are formed elementwise from them on the inputs as given."""
    from avvad import ops
    e, r, v = _on_gpu(s_hat, s, n)
    _, alpha = ops.energy_ratios(e, r, noise=v, return_alpha=True)
    if all(isinstance(x, np.ndarray) for x in (s_hat, s, n)):
        a_s, a_n = (float(a) for a in alpha[0].tolist())
    else:
        import torch
        s_hat, s, n = (x if isinstance(x, torch.Tensor) else torch.as_tensor(x) for x in (s_hat, s, n))
        a_s, a_n = alpha[0, 0].to(s.device), alpha[0, 1].to(n.device)
    s_target = a_s * s
    e_noise = a_n * n
    return s_target, e_noise, s_hat - s_target - e_noise


def energy_ratios(s_hat, s, n):
    """(si_sdr, si_sir, si_sar) in dB (``si_sir`` is the reference's name for the SI-SNR: noise is the only interferer):
    floats for numpy input, 0-dim float64 tensors on the GPU for tensor input."""
    import torch
    from avvad import ops
    e, r, v = _on_gpu(s_hat, s, n)
    ratios = ops.energy_ratios(e, r, noise=v)[0]
    if any(isinstance(x, torch.Tensor) for x in (s_hat, s, n)):
        return ratios[0], ratios[1], ratios[2]
    return tuple(float(x) for x in ratios.tolist())


def stoi(x, y, fs_sig=16000, extended=False):
    """STOI (``extended``: ESTOI) of the processed signal ``y`` against the clean ``x``, the call of the Python package the
    field uses: numpy arrays in, a Python float out.  Runs on the GPU (``avvad.ops.stoi``, csrc/stoi.hip); ``fs_sig`` is
    16000 or 10000."""
    from avvad import ops
    c, p = _on_gpu(x, y)
    if c.numel() != p.numel():
        raise ValueError("x and y should have the same length, found %d and %d" % (c.numel(), p.numel()))
    return float(ops.stoi(c, p, fs=fs_sig, extended=extended)[0])


def mean_confidence_interval(data, confidence=0.95, round=3):
    """(mean, half-width of the two-sided Student-t interval), both rounded to 3 decimals -- the reference
    ignores its ``round`` argument (``:10``) and so does this."""
    a = np.asarray(data, dtype=np.float64)
    n = a.shape[0]
    half = scipy.stats.sem(a) * scipy.stats.t.ppf(0.5 * (1.0 + confidence), n - 1)
    return np.round(a.mean(), 3), np.round(half, 3)


def _table(columns, rows, confidence):
    """columns: {name: per-utterance values}; rows: index array / mask selecting the utterances of this table."""
    print("{:<10} {:<10} {:<10}".format('METRIC', 'AVERAGE', 'CONF. INT.'))
    out = {}
    for name, values in columns.items():
        m, h = mean_confidence_interval(np.asarray(values)[rows], confidence=confidence)
        out[name] = {'avg': m, '+/-': h}
        print("{:<10} {:<10} {:<10}".format(name, m, h))
    print('\n')
    return out


def compute_stats(metrics_keys, all_metrics, model_data_dir, confidence, all_snr_db=None, all_noise_types=None,
                  all_speakers=None):
    """all_metrics: one tuple of scores per utterance, in ``metrics_keys`` order.  Prints the overall table, then one
    table per distinct SNR / noise type / speaker when those per-utterance labels are given (SNRs ascending as in the
    reference; noise types and speakers in sorted order -- the reference iterates a ``set``).  ``model_data_dir`` is
    accepted for signature compatibility (the reference's json dump is commented out, ``:83-85``)."""
    n = len(all_metrics)
    columns = {key: np.array([row[j] for row in all_metrics], dtype=np.float64) for j, key in enumerate(metrics_keys)}
    stats = {'all': _table(columns, np.arange(n), confidence)}
    groups = (('Input SNR = {:.2f}', all_snr_db, 'snr'), ('Noise type = {}', all_noise_types, 'noise'),
              ('Speaker = {}', all_speakers, 'speaker'))
    for title, labels, tag in groups:
        if labels is None:
            continue
        labels = np.asarray(labels)
        for value in np.unique(labels):
            print(title.format(value))
            stats[(tag, value.item() if hasattr(value, 'item') else value)] = _table(columns, labels == value, confidence)
    return stats
