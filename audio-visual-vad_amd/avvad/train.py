"""Training / evaluation loops shared by the ``scripts/train_*.py`` and ``scripts/evaluate_*.py`` entry points.

They mirror the loop bodies of the reference (``scripts/train_AV_net.py:252-448``, ``train_audio_net.py:190-372``,
``train_video_net.py:182-319``, ``evaluate_AV_net.py:148-250``): per batch -- move to the GPU, standardise with the
train-set statistics when given (``std_norm``: ``(x - mean.T) / (std + eps).T``, ``train_AV_net.py:286-291``), forward,
per-sequence masked BCE summed over the batch, backward, Adam, per-sequence accuracy/precision/recall/F1 -- with the
reference's Python loops over the batch replaced by single fused calls, ``nn.DataParallel`` replaced by one process per
GPU + bucketed RCCL all-reduce, and a synthetic data source for training (the reference's HDF5 readers are out of scope,
SURVEY.md 2.1; h5py and torchaudio are not installed in this image), (noisy, clean) wav pairs whose labels are computed
on the GPU from the clean files (``WavPairs``, ``wav_pair_step``), or such pairs with the utterance's lip-region DCT
coefficients, decoded to video frames on the GPU (``AVFiles``, ``av_file_step``).  Clean utterances can also be mixed
with clips of a noise bank at a drawn SNR in the step itself (``CleanWavs``, ``mix_step``, ``ops.mix``).  On wav pairs a 513-bin mask model can
be trained on the SI-SDR of its resynthesised waveform instead of the BCE (``objective="si_sdr"``, ``SiSdrObjective``).  The per-utterance evaluator of the audio network
(``process_utt``, ``evaluate_audio_net.py:107-180``) runs the reference's whole chain on real waveforms: peak
normalisation -> STFT -> power -> log -> crop to the label length -> standardise -> classifier -> sigmoid -> threshold."""
import math
import os
import time

import torch

from . import dist as avd
from . import ops
from . import stream
from .optim import FlatAdam

EPS = 1e-8


class Stats:
    """Train-set mean / std used by ``std_norm`` (the reference reads them from HDF5 and saves ``trainset_*_mean.npy``,
    ``train_AV_net.py:206-231``): audio (513,1) per-bin vectors, video (1,1) scalars."""

    def __init__(self, audio_mean=None, audio_std=None, video_mean=None, video_std=None, eps=EPS):
        self.eps = eps
        self._raw = dict(audio_mean=audio_mean, audio_std=audio_std, video_mean=video_mean, video_std=video_std)
        self._dev = {}

    @classmethod
    def load(cls, model_dir, eps=EPS):
        """``trainset_{audio,video}_{mean,std}.npy`` as the reference's training script writes them."""
        import numpy as np
        kw = {}
        for k in ("audio_mean", "audio_std", "video_mean", "video_std"):
            path = os.path.join(model_dir, "trainset_%s.npy" % k)
            if os.path.exists(path):
                kw[k] = np.load(path, allow_pickle=False)
        return cls(eps=eps, **kw)

    def save(self, model_dir):
        """Writes the statistics this object holds as ``trainset_{audio,video}_{mean,std}.npy`` in the shapes the
        reference writes and ``load`` reads -- (513, 1) per-bin columns, (1, 1) scalars, float32 -- and returns
        ``model_dir``: ``Stats.load(stats.save(d))`` holds the same values bit for bit."""
        import numpy as np
        os.makedirs(model_dir, exist_ok=True)
        for k, v in self._raw.items():
            if v is not None:
                v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
                np.save(os.path.join(model_dir, "trainset_%s.npy" % k), np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 1))
        return model_dir

    def get(self, key, device):
        if self._raw.get(key) is None:
            return None
        if (key, device) not in self._dev:
            self._dev[(key, device)] = torch.as_tensor(self._raw[key], dtype=torch.float32).reshape(-1).to(device)
        return self._dev[(key, device)]

    def audio(self, x):
        m, s = self.get("audio_mean", x.device), self.get("audio_std", x.device)
        return x if m is None else ops.standardize(x, m, s, self.eps)

    def video(self, v):
        m, s = self.get("video_mean", v.device), self.get("video_std", v.device)
        return v if m is None else ops.standardize(v, m, s, self.eps)


class SyntheticAV(torch.utils.data.Dataset):
    """Items shaped like the reference's datasets return them (``data_handling.py:387-495``): audio features
    (513, T) or a waveform (L,), video (67, 67, T), target (1, T), [L,] T -- ragged T per item."""

    def __init__(self, n_items, kind, t_min=8, t_max=16, waveform=False, rf=2048, seed=0):
        self.n, self.kind, self.t_min, self.t_max, self.waveform, self.rf, self.seed = n_items, kind, t_min, t_max, waveform, rf, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 100003 + i)
        T = int(torch.randint(self.t_min, self.t_max + 1, (1,), generator=g))
        y = (torch.rand(1, T, generator=g) > 0.5).float()
        item = []
        L = T * 256 + self.rf - 1
        if self.kind in ("audio", "av"):
            if self.waveform:
                w = torch.rand(L, generator=g) * 2 - 1
                item.append(w / w.abs().max())
            else:
                item.append(torch.randn(513, T, generator=g))
        if self.kind in ("video", "av"):
            item.append(torch.randn(67, 67, T, generator=g))
        item.append(y)
        if self.waveform and self.kind != "video":
            item.append(L)
        item.append(T)
        return tuple(item)


def pick_collate(kind, waveform):
    from packages import utils as U
    if kind == "audio":
        return U.collate_many2many_audio_waveform if waveform else U.collate_many2many_audio
    if kind == "video":
        return U.collate_many2many_video
    return U.collate_many2many_AV_waveform if waveform else U.collate_many2many_AV


class WavPairs(torch.utils.data.Dataset):
    """(noisy, clean) 16 kHz wav pairs laid out like NTCD-TIMIT -- what the reference's
    ``NoisyWavWholeSequenceSpectrogramLabeledFrames`` reads (``data_handling.py:231-320``), with the labels computed from
    the clean file in the training step (``wav_pair_step``) instead of read from HDF5.  ``pairs``: a list of
    (noisy path, clean path) or a text file with one "noisy clean" pair per line.  Items: (noisy (L,), clean (L,), L),
    both cropped to their common length.  ``resample``: files of other rates are allowed (the two of a pair may differ);
    items are then (noisy (Ln,), clean (Lc,), Ln, Lc, noisy rate, clean rate) as read, and the training step resamples them
    on the GPU (``to_16k``) before it crops them to their common length."""

    def __init__(self, pairs, resample=False):
        self.pairs = read_wav_pairs(pairs) if isinstance(pairs, str) else [tuple(p) for p in pairs]
        self.resample = bool(resample)

    def __len__(self):
        return len(self.pairs)

    def __getitem__(self, i):
        noisy_path, clean_path = self.pairs[i]
        noisy, fs_n = load_waveform(noisy_path)
        clean, fs_c = load_waveform(clean_path)
        if self.resample:
            return noisy, clean, noisy.numel(), clean.numel(), int(fs_n), int(fs_c)
        if fs_n != 16000 or fs_c != 16000:
            raise ValueError("%s / %s: expected 16 kHz audio, got %d / %d Hz" % (noisy_path, clean_path, fs_n, fs_c))
        n = min(noisy.numel(), clean.numel())
        return noisy[:n], clean[:n], n

    @staticmethod
    def collate(batch):
        """-> (sample lengths LongTensor (B,), noisy (B, Lmax), clean (B, Lmax)), rows zero-padded.  Items that carry
        their rates (``resample=True``): lengths (B, 2) -- noisy, clean -- each signal padded to its own longest row, and a
        trailing ``rates`` LongTensor (B, 2)."""
        if len(batch[0]) == 6:
            noisy = torch.zeros(len(batch), max(item[2] for item in batch))
            clean = torch.zeros(len(batch), max(item[3] for item in batch))
            for i, item in enumerate(batch):
                noisy[i, :item[2]] = item[0]
                clean[i, :item[3]] = item[1]
            return (torch.LongTensor([[item[2], item[3]] for item in batch]), noisy, clean,
                    torch.LongTensor([[item[4], item[5]] for item in batch]))
        lens = [item[2] for item in batch]
        noisy = torch.zeros(len(batch), max(lens))
        clean = torch.zeros(len(batch), max(lens))
        for i, (nz, cl, n) in enumerate(batch):
            noisy[i, :n] = nz
            clean[i, :n] = cl
        return torch.LongTensor(lens), noisy, clean


def read_wav_pairs(path):
    """A text file with one "noisy clean" pair of paths per line (blank lines and # comments skipped)."""
    pairs = []
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].strip()
            if line:
                noisy, clean = line.split()
                pairs.append((noisy, clean))
    return pairs


def labels_for_ydim(y_dim):
    """The reference's scripts tie the label kind to the head's width (create_audio_train_files.py:87-90)."""
    if y_dim == 1:
        return "vad_labels"
    if y_dim == 513:
        return "ibm_labels"
    raise ValueError("y_dim %d: wav-pair labels are VAD (y_dim 1) or IBM (y_dim 513)" % y_dim)


def wav_pair_step(batch, device, labels, stats=None, fs=16e3, wlen_sec=64e-3, hop_percent=0.25, eps=EPS, waves=False):
    """A ``WavPairs.collate`` batch -> (frame lengths, features (B, T, 513), target (B, T, y_dim)) on the GPU: every file
    peak-normalised on its own (``x / max|x|``, as the reference normalises each file it reads), log-power STFT features of
    the noisy file (standardised when ``stats`` hold the train-set statistics), labels of the clean file with the training
    pipeline's settings (64 ms, hop 0.25, ``center=False``, end pad; create_audio_train_files.py:44-60) and the same
    frame counts.  ``waves``: a fourth value, (peak-normalised noisy (B, L), clean (B, L), sample lengths), what a loss on
    the resynthesised waveform needs."""
    lens, noisy, clean = pair_waves(batch, device)
    noisy = ops.peak_normalize(noisy)
    clean = ops.peak_normalize(clean)
    return _pair_tail(lens, noisy, clean, device, labels, stats, fs, wlen_sec, hop_percent, eps, waves)


def to_16k(waves, lens, rates, device):
    """A ragged batch of mixed rates -> (waves16 (B, Lmax16) on the GPU, lens16 (list)): waves (B, Lmax) float32 (host or
    GPU), row b holding ``lens[b]`` samples at ``rates[b]`` Hz.  One ragged ``ops.resample`` call per distinct rate in the
    batch; 16 kHz rows are copied; the rows go back in their order, zeros behind each row's samples."""
    lens, rates = [int(v) for v in lens], [int(r) for r in rates]
    B = len(lens)
    if len(rates) != B or tuple(waves.shape[:1]) != (B,) or waves.dim() != 2:
        raise ValueError("to_16k: waves (B, Lmax) with one length and one rate per row, got %s, %d lengths, %d rates"
                         % (tuple(waves.shape), B, len(rates)))
    w = waves.to(device, non_blocking=True)
    groups = {}
    for b, r in enumerate(rates):
        groups.setdefault(r, []).append(b)
    lens16, parts = list(lens), []
    for r, rows in groups.items():
        Lg = max(lens[b] for b in rows)
        if r == 16000 or Lg == 0:
            parts.append((rows, w[rows][:, :Lg] if len(rows) < B else w[:, :Lg]))
            continue
        out, n = ops.resample(w[rows][:, :Lg] if len(rows) < B else w[:, :Lg], [lens[b] for b in rows], fs_in=r)
        for b, k in zip(rows, n):
            lens16[b] = k
        parts.append((rows, out))
    if len(parts) == 1 and parts[0][1].shape[1] == max(lens16):
        return parts[0][1], lens16
    out16 = torch.zeros(B, max(lens16), dtype=torch.float32, device=w.device)
    for rows, part in parts:
        k = min(part.shape[1], out16.shape[1])
        out16[torch.tensor(rows, device=w.device), :k] = part[:, :k]
    return out16, lens16


def _crop_rows(w, lens, n):
    """w (B, >= max(n)) whose row b holds lens[b] samples -> (B, max(n)) with zeros from n[b] <= lens[b] on"""
    w = w[:, :max(n)]
    if all(a == b for a, b in zip(lens, n)):
        return w.contiguous()
    keep = torch.arange(w.shape[1], device=w.device)[None, :] < torch.tensor(n, device=w.device)[:, None]
    return torch.where(keep, w, torch.zeros((), dtype=w.dtype, device=w.device))


def pair_waves(batch, device):
    """A ``WavPairs.collate`` batch on the GPU -> (sample lengths (LongTensor), noisy (B, L), clean (B, L)).  A batch
    that carries rates is resampled (``to_16k``) and each pair cropped to its common length first."""
    if len(batch) == 3:
        lens, noisy, clean = batch
        return lens, noisy.to(device, non_blocking=True), clean.to(device, non_blocking=True)
    lens, noisy, clean, rates = batch
    noisy, ln = to_16k(noisy, lens[:, 0], rates[:, 0], device)
    clean, lc = to_16k(clean, lens[:, 1], rates[:, 1], device)
    n = [min(a, b) for a, b in zip(ln, lc)]
    return torch.LongTensor(n), _crop_rows(noisy, ln, n), _crop_rows(clean, lc, n)


def clean_waves(batch, device):
    """A ``CleanWavs.collate`` batch on the GPU -> (sample lengths (LongTensor), clean (B, L)), resampled (``to_16k``) when
    the batch carries rates."""
    if len(batch) == 2:
        return batch[0], batch[1].to(device, non_blocking=True)
    lens, clean, rates = batch
    clean, n = to_16k(clean, lens, rates, device)
    return torch.LongTensor(n), clean


def _pair_tail(lens, noisy, clean, device, labels, stats, fs, wlen_sec, hop_percent, eps, waves, more=(), made=None):
    """What ``wav_pair_step`` and ``mix_step`` share, from the peak-normalised noisy and clean waves on: the labels of the
    clean wave, the features of the noisy one, the frame-count check.  ``more``: further members of the ``waves`` tuple.
    ``made``: (frame lengths, target) made by the caller; no clean-speech label is computed then."""
    frames, target = made if made is not None else ops.speech_targets(
        clean, lens, labels, fs=fs, wlen_sec=wlen_sec, hop_percent=hop_percent, center=False, pad_at_end=True, eps=eps)
    nfft = int(wlen_sec * fs)
    mean = std = None
    if stats is not None:
        mean, std = stats.get("audio_mean", device), stats.get("audio_std", device)
    x = ops.stft(noisy, nfft, int(hop_percent * nfft), mode=0, eps=eps, pad_at_end=True, fs=fs, mean=mean, std=std,
                 norm_eps=stats.eps if stats is not None else eps)
    T = target.shape[1]
    if x.shape[1] != T:                 # the longest row's frame count on both sides (same lengths, same rule)
        raise RuntimeError("feature frames %d != label frames %d" % (x.shape[1], T))
    if waves:
        return frames.to(device), x, target, (noisy, clean, [int(n) for n in lens]) + tuple(more)
    return frames.to(device), x, target


class CleanWavs(torch.utils.data.Dataset):
    """Clean 16 kHz utterances to be mixed with noise in the training step (``mix_step``).  ``paths``: a list of paths or
    a text file with one path per line (blank lines and # comments skipped).  Items: (clean (L,), L).  ``resample``:
    files of other rates are allowed; items are then (clean (L,), L, rate) as read and ``mix_step`` resamples them on the
    GPU (``to_16k``)."""

    def __init__(self, paths, resample=False):
        self.paths = read_path_list(paths) if isinstance(paths, str) else [str(p) for p in paths]
        self.resample = bool(resample)

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        clean, fs = load_waveform(self.paths[i])
        if self.resample:
            return clean, clean.numel(), int(fs)
        if fs != 16000:
            raise ValueError("%s: expected 16 kHz audio, got %d Hz" % (self.paths[i], fs))
        return clean, clean.numel()

    @staticmethod
    def collate(batch):
        """-> (sample lengths LongTensor (B,), clean (B, Lmax)), rows zero-padded; a trailing ``rates`` LongTensor (B,)
        when the items carry their rate (``resample=True``)."""
        lens = [item[1] for item in batch]
        clean = torch.zeros(len(batch), max(lens))
        for i, item in enumerate(batch):
            clean[i, :item[1]] = item[0]
        if len(batch[0]) == 3:
            return torch.LongTensor(lens), clean, torch.LongTensor([item[2] for item in batch])
        return torch.LongTensor(lens), clean


def read_path_list(path):
    """A text file with one path per line (blank lines and # comments skipped)."""
    with open(path) as f:
        return [line for line in (raw.split("#", 1)[0].strip() for raw in f) if line]


def read_noise_bank(paths, device, resample=False):
    """The noise clips of ``paths`` (a list, or a text file with one path per line) as an ``ops.NoiseBank`` on ``device``:
    every file read with ``load_waveform``, 16 kHz enforced, not normalised (the mix sets each row's gain).  ``resample``:
    a clip of another rate is resampled on the GPU (``ops.resample``) once, before it enters the bank."""
    clips = []
    for p in (read_path_list(paths) if isinstance(paths, str) else list(paths)):
        x, fs = load_waveform(str(p))
        if fs != 16000 and resample:
            x = ops.resample(x.to(device), fs_in=fs)[0]
        elif fs != 16000:
            raise ValueError("%s: expected 16 kHz audio, got %d Hz" % (p, fs))
        clips.append(x)
    return ops.NoiseBank(clips, device)


def mix_generator(mix_seed, epoch, rank):
    """The host generator of one pass of mixtures, seeded by (mix_seed, epoch, rank); ``epoch`` is a number or a name
    ("valid", "stats").  The seed is the first 63 bits of a SHA-256 of the triple: the same on every machine, and no two
    triples share a stream by arithmetic accident."""
    import hashlib
    key = repr((int(mix_seed), epoch if isinstance(epoch, str) else int(epoch), int(rank))).encode()
    return torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(key).digest()[:8], "little") >> 1)


def snr_range(snr_db):
    """(lo, hi) in dB as floats from a pair or a single number; anything but a finite range with lo <= hi is a ValueError."""
    try:
        lo, hi = (snr_db, snr_db) if isinstance(snr_db, (int, float)) else snr_db
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError("snr_db %r: a number or a (lo, hi) pair in dB" % (snr_db,))
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError("snr_db %r: a finite (lo, hi) range in dB with lo <= hi" % (snr_db,))
    return lo, hi


def draw_mix(gen, lengths, bank, snr_db):
    """One draw per row of a batch from the host generator ``gen``: a clip of ``bank`` (uniform over the clips), a start
    within it (uniform over its samples) and an SNR uniform in ``snr_db = (lo, hi)`` dB (a single number: that SNR).
    ``lengths``: the batch's sample lengths (their count is the batch size).  -> (clip, start, snr_db), lists of B."""
    B = len(lengths)
    lo, hi = snr_range(snr_db)
    clip = torch.randint(0, bank.K, (B,), generator=gen).tolist()
    u = torch.rand(2, B, dtype=torch.float64, generator=gen)
    start = [min(int(float(u[0, b]) * bank.lengths[k]), bank.lengths[k] - 1) for b, k in enumerate(clip)]
    snr = [lo + (hi - lo) * float(u[1, b]) for b in range(B)]
    return clip, start, snr


class MixDraw:
    """The ``draw`` of ``mix_step`` in ``train_main``: ``seed(epoch)`` starts the pass (mix_seed, epoch, rank), every call
    then draws one batch's (clip, start, snr_db) from it in the order the batches arrive."""

    def __init__(self, bank, snr_db, mix_seed=0, rank=0):
        self.bank, self.snr_db, self.mix_seed, self.rank = bank, snr_db, mix_seed, rank
        self.gen = None

    def seed(self, epoch):
        self.gen = mix_generator(self.mix_seed, epoch, self.rank)
        return self

    def __call__(self, lengths):
        if self.gen is None:
            raise RuntimeError("MixDraw.seed(epoch) starts a pass of mixtures")
        return draw_mix(self.gen, lengths, self.bank, self.snr_db)


MIX_LABELS = {"clean": None, "noise_aware": "speech", "irm": "irm"}      # -> the output of ops.noise_aware_targets


def check_mix_labels(mix_labels, mixing, y_dim=None):
    """``mix_labels`` "noise_aware" and "irm" label a mixture made in the step (``mixing``: clean_wavs / noise_wavs are
    given) for a 513-bin mask head; anything else is a ValueError (``y_dim`` None: not known yet)."""
    if mix_labels not in MIX_LABELS:
        raise ValueError("mix_labels %r: one of %s" % (mix_labels, ", ".join(MIX_LABELS)))
    if mix_labels != "clean":
        if not mixing:
            raise ValueError("mix_labels %r needs the noise of the mixture: it goes with clean_wavs / noise_wavs" % mix_labels)
        if y_dim is not None and y_dim != 513:
            raise ValueError("mix_labels %r are 513-bin masks (y_dim 513), got y_dim %d" % (mix_labels, y_dim))


def mix_step(batch, device, labels, bank, draw, stats=None, fs=16e3, wlen_sec=64e-3, hop_percent=0.25, eps=EPS, waves=False,
             mix_labels="clean", peak=False):
    """A ``CleanWavs.collate`` batch -> what ``wav_pair_step`` returns, with a mixture made in the step in place of the noisy
    file: the clean waves are peak-normalised, ``draw(lengths)`` gives every row a clip of ``bank``, a start and an SNR
    in dB (``draw_mix``), ``ops.mix`` adds the noise at that SNR on the GPU, and the mixture is peak-normalised like a
    noisy file that was read.  ``waves``: the fourth value is (peak-normalised mixture (B, L), clean (B, L), sample
    lengths, noise (B, L)) -- the noise as it was added, ``g_b n``, on the scale of the mixture BEFORE its
    normalisation (SI-SIR and SI-SAR do not depend on that scale).
    ``mix_labels``: "clean" labels the clean wave alone (``labels``); "noise_aware" / "irm" (``labels`` "ibm_labels" only)
    take the target from the mixture's two components instead -- the speech mask of ``noise_aware_IBM`` or the ideal ratio
    mask of (clean, ``g_b n``), both over the mixture's peak, i.e. on the scale of the normalised mixture the model sees
    (``ops.noise_aware_targets``) -- and compute no clean-speech label.
    ``peak`` (with ``waves``): a fifth member of that tuple, the (B,) peak of the mixture before its normalisation
    (``ops.mix``'s ``info["peak"]``), the scale a spectrum-approximation loss puts the clean spectrum on."""
    check_mix_labels(mix_labels, True)
    if mix_labels != "clean" and labels != "ibm_labels":
        raise ValueError("mix_labels %r are 513-bin masks: they go with labels 'ibm_labels', got %r" % (mix_labels, labels))
    lens, clean = clean_waves(batch, device)
    clean = ops.peak_normalize(clean)
    n = [int(v) for v in lens]
    clip, start, snr = draw(n)
    made = None
    if mix_labels == "clean" and not peak:
        mixed = ops.mix(clean, n, bank, clip, start, snr, return_noise=waves)
        noisy, more = (mixed[0], (mixed[1],)) if waves else (mixed, ())
    else:
        noisy, noise, info = ops.mix(clean, n, bank, clip, start, snr, return_noise=True, return_info=True)
        if mix_labels != "clean":
            which = MIX_LABELS[mix_labels]
            frames, out = ops.noise_aware_targets(clean, noise, n, peak=info["peak"], outputs=(which,), fs=fs, wlen_sec=wlen_sec,
                                                  hop_percent=hop_percent, pad_at_end=True)
            made = (frames, out[which])
        more = ((noise,) if waves else ()) + ((info["peak"],) if waves and peak else ())
    return _pair_tail(lens, ops.peak_normalize(noisy), clean, device, labels, stats, fs, wlen_sec, hop_percent, eps, waves, more,
                      made)


SPECTRAL_OBJECTIVES = {"mse_mask": "mask", "mse_signal": "signal", "msa": "spectrum"}      # -> the kind of ops.spectral_loss
STOI_OBJECTIVES = {"stoi": False, "estoi": True}                                            # -> ops.stoi_loss's ``extended``
OBJECTIVES = ("bce", "si_sdr") + tuple(SPECTRAL_OBJECTIVES) + tuple(STOI_OBJECTIVES)


def check_objective(objective, kind, waveform, wav_pairs, y_dim=None, clean_wavs=None):
    """``objective`` "si_sdr" trains a 513-bin mask model of the audio network on wav pairs, or on clean utterances mixed
    with noise in the step (``clean_wavs``), and so do the mask-regression objectives "mse_mask", "mse_signal" and "msa";
    "stoi" and "estoi" train under the conditions of "si_sdr"; anything else is a ValueError (``y_dim`` None: not known yet)."""
    if objective not in OBJECTIVES:
        raise ValueError("objective %r: one of %s" % (objective, ", ".join(OBJECTIVES)))
    if objective in SPECTRAL_OBJECTIVES:
        if kind != "audio" or waveform or (wav_pairs is None and clean_wavs is None):
            raise ValueError("objective %r trains the audio network on spectrograms of wav_pairs, or of clean_wavs mixed with "
                             "noise_wavs: it regresses the model's mask onto the step's label or spectra" % objective)
        if y_dim is not None and y_dim != 513:
            raise ValueError("objective %r needs a 513-bin mask head (y_dim 513), got y_dim %d" % (objective, y_dim))
    if objective == "si_sdr":
        if kind != "audio" or waveform or (wav_pairs is None and clean_wavs is None):
            raise ValueError("objective 'si_sdr' trains the audio network on spectrograms of wav_pairs: it resynthesises "
                             "the noisy file through the model's mask")
        if y_dim is not None and y_dim != 513:
            raise ValueError("objective 'si_sdr' needs a 513-bin mask head (y_dim 513), got y_dim %d" % y_dim)
    if objective in STOI_OBJECTIVES:
        if kind != "audio" or waveform or (wav_pairs is None and clean_wavs is None):
            raise ValueError("objective %r trains the audio network on spectrograms of wav_pairs, or of clean_wavs mixed with "
                             "noise_wavs: it resynthesises the noisy wave through the model's mask" % objective)
        if y_dim is not None and y_dim != 513:
            raise ValueError("objective %r needs a 513-bin mask head (y_dim 513), got y_dim %d" % (objective, y_dim))


class SiSdrObjective:
    """The step of ``objective="si_sdr"``: ``prepare`` is ``wav_pair_step`` and keeps the batch's waves, ``loss`` resynthesises
    the noisy wave through sigmoid(logits) (``ops.resynth``, mask_mode 2) and returns minus the summed SI-SDR against the
    clean wave (``ops.si_sdr_loss``) -- summed over the batch like the BCE -- and the batch's mean SI-SDR for the log line.
    The first and last ``n_fft - hop`` samples of every utterance stay out of the loss: with ``center=False`` they divide by
    a window sum of squares that falls to 1e-10, and a masked estimate there would own it."""

    def __init__(self, device, labels, stats, fs=16e3, wlen_sec=64e-3, hop_percent=0.25, step=None):
        self.device, self.labels, self.stats = device, labels, stats      # stats: a callable, read at every step
        self.fs, self.wlen_sec, self.hop_percent = fs, wlen_sec, hop_percent
        self.n_fft = int(wlen_sec * fs)
        self.hop = int(hop_percent * self.n_fft)
        self.waves = None
        self.step = step                  # (batch, stats) -> wav_pair_step's four values (mix_step); None: wav pairs

    def prepare(self, batch):
        if self.step is not None:
            frames, x, target, self.waves = self.step(batch, self.stats())
        else:
            frames, x, target, self.waves = wav_pair_step(batch, self.device, self.labels, self.stats(), self.fs, self.wlen_sec,
                                                          self.hop_percent, waves=True)
        return frames, x, target

    def estimate(self, logits):
        noisy, _, lens = self.waves[:3]
        return ops.resynth(noisy, logits, mask_mode=2, n_fft=self.n_fft, hop=self.hop, sample_lengths=lens, pad_at_end=True, fs=self.fs)

    def loss(self, logits, y, lengths):
        _, clean, lens = self.waves[:3]
        est = self.estimate(logits)
        skip = self.n_fft - self.hop
        loss, ratios = ops.si_sdr_loss(est, clean, lens, skip, skip, return_ratios=True)
        return loss, "  si-sdr %.2f dB" % float(torch.nanmean(ratios))


class StoiObjective(SiSdrObjective):
    """The step of ``objective="stoi"`` / ``"estoi"``: ``SiSdrObjective``'s ``prepare`` and resynthesis, then minus the summed
    STOI (``extended``: ESTOI) of the estimate against the clean wave (``ops.stoi_loss``), and the batch's mean score for the
    log line.  The same first and last ``n_fft - hop`` samples stay out, for ``SiSdrObjective``'s reason: the two waves are
    sliced (the op takes pitched views) and every length loses both margins."""

    def __init__(self, objective, device, labels, stats, fs=16e3, wlen_sec=64e-3, hop_percent=0.25, step=None):
        super().__init__(device, labels, stats, fs, wlen_sec, hop_percent, step)
        self.name, self.extended = objective, STOI_OBJECTIVES[objective]

    def loss(self, logits, y, lengths):
        _, clean, lens = self.waves[:3]
        est = self.estimate(logits)
        skip = self.n_fft - self.hop
        n = min(est.shape[1], clean.shape[1])
        inner = [max(0, min(int(v), n) - 2 * skip) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
        loss, d = ops.stoi_loss(est[:, skip:n], clean[:, skip:n], inner, fs=int(self.fs), extended=self.extended, return_scores=True)
        return loss, "  %s %.6f" % (self.name, float(d.mean()))


class SpectralObjective:
    """The step of the mask-regression objectives "mse_mask", "mse_signal" and "msa" (``ops.spectral_loss`` on
    sigmoid(logits), summed over the batch like the BCE).  ``prepare`` is ``wav_pair_step`` -- or ``step``, ``mix_step``
    with ``waves`` and ``peak`` -- and keeps what the loss needs:
      "mse_mask", "mse_signal": the step's own label -- the IBM of the clean wave, or the noise-aware mask / IRM of a mixture;
      "mse_signal", "msa":      X = ``ops.stft_complex`` of the peak-normalised mixture, the one the features come from;
      "msa":                    S = ``ops.stft_complex`` of the clean wave over the MIXTURE's peak, not its own, so that S
                                and X are on one scale (the reference's metrics script scales ``s_t / norm_max`` the same
                                way).  For a mixture made in the step that peak is ``ops.mix``'s ``info["peak"]`` and the
                                clean wave is the one the noise was added to; for a wav pair it is the noisy file's
                                ``abs_max`` and the clean wave is the clean file as read.
    The spectra's frame count must be the features' (``_pair_tail``'s check).  ``loss`` returns the summed loss and the
    batch's mean per-utterance loss for the log line."""

    def __init__(self, objective, device, labels, stats, fs=16e3, wlen_sec=64e-3, hop_percent=0.25, step=None):
        self.kind = SPECTRAL_OBJECTIVES[objective]
        self.name = objective
        self.device, self.labels, self.stats = device, labels, stats      # stats: a callable, read at every step
        self.fs, self.wlen_sec, self.hop_percent = fs, wlen_sec, hop_percent
        self.n_fft = int(wlen_sec * fs)
        self.hop = int(hop_percent * self.n_fft)
        self.step = step                  # (batch, stats) -> mix_step's four values with the peak; None: wav pairs
        self.mix = self.speech = None

    def _spectrum(self, wave, T):
        spec = ops.stft_complex(wave, self.n_fft, self.hop, pad_at_end=True, fs=self.fs)
        if spec.shape[1] != T:
            raise RuntimeError("spectrum frames %d != label frames %d" % (spec.shape[1], T))
        return spec

    def prepare(self, batch):
        if self.step is not None:
            frames, x, target, (noisy, clean, _lens, _noise, peak) = self.step(batch, self.stats())
        else:
            lens, noisy, clean = pair_waves(batch, self.device)
            peak = ops.peak(noisy)
            frames, x, target, (noisy, _clean, _lens) = _pair_tail(
                lens, ops.peak_normalize(noisy), ops.peak_normalize(clean), self.device, self.labels, self.stats(), self.fs,
                self.wlen_sec, self.hop_percent, EPS, True)
        T = target.shape[1]
        self.mix = self._spectrum(noisy, T) if self.kind != "mask" else None
        self.speech = None
        if self.kind == "spectrum":         # (a silent mixture has nothing to scale by: its clean wave stays as it is)
            scale = torch.where(peak > 0, 1.0 / peak, torch.ones_like(peak))
            self.speech = self._spectrum(clean * scale[:, None], T)
        return frames, x, target

    def loss(self, logits, y, lengths):
        loss, rows = ops.spectral_loss(logits, self.kind, target=y if self.kind != "spectrum" else None, mix=self.mix,
                                       speech=self.speech, lengths=lengths, pred_mode=2, return_rows=True)
        return loss, "  %s/utt %.4f" % (self.name, float(rows.mean()))


def rank_shard(n, rank, world):
    """The items rank ``rank`` of ``world`` takes out of ``n``: every item belongs to exactly one rank."""
    return range(rank, n, world)


def merge_stats(accs):
    """Sum of statistics accumulators (``ops.stats_new`` layout: sums, sums of squares, count), added in the given order:
    accumulating a set in parts and merging equals accumulating it in one up to double rounding of the additions."""
    accs = list(accs)
    out = accs[0].clone()
    for a in accs[1:]:
        out += a
    return out


def wav_pair_stats(pairs, device, batch_size=16, fs=16e3, wlen_sec=64e-3, hop_percent=0.25, eps=EPS, resample=False):
    """Train-set statistics of the audio features over (noisy, clean) wav pairs -> ``Stats`` (audio (513, 1) mean / std):
    what ``create_audio_train_files.py:196-214, 340-392`` computes offline.  ``pairs``: a ``WavPairs``, a list of pairs or
    a text file of them.  Every noisy file is peak-normalised as ``wav_pair_step`` does and its log-power STFT frames --
    the frame counts ``wav_pair_step`` uses -- are accumulated on the GPU without materialising the features
    (``ops.stft_stats``).  With ``torch.distributed`` initialised every rank takes ``rank_shard`` of the pairs and the
    float64 accumulators are summed by one all-reduce.  ``resample``: as ``WavPairs``'s (a ``WavPairs`` brings its own)."""
    import torch.distributed as dist
    if not isinstance(pairs, WavPairs):
        pairs = WavPairs(pairs, resample)
    multi = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(), dist.get_world_size()) if multi else (0, 1)
    nfft = int(wlen_sec * fs)
    acc = ops.stats_new(nfft // 2 + 1, device)
    loader = torch.utils.data.DataLoader(torch.utils.data.Subset(pairs, rank_shard(len(pairs), rank, world)),
                                         batch_size=batch_size, shuffle=False, collate_fn=WavPairs.collate)
    for batch in loader:
        lens, noisy, _ = pair_waves(batch, device)
        noisy = ops.peak_normalize(noisy)
        ops.stft_stats(acc, noisy, lens, nfft, int(hop_percent * nfft), eps=eps, pad_at_end=True, fs=fs)
    if multi:
        dist.all_reduce(acc)                 # the merge across ranks: merge_stats of the ranks' accumulators
    mean, std = ops.finalize_stats(acc)
    return Stats(audio_mean=mean.cpu().numpy().reshape(-1, 1), audio_std=std.cpu().numpy().reshape(-1, 1), eps=eps)


def mix_stats(clean, bank, device, draw, batch_size=16, fs=16e3, wlen_sec=64e-3, hop_percent=0.25, eps=EPS, resample=False):
    """``wav_pair_stats`` over mixtures made on the fly: one pass over the clean utterances (``clean``: a ``CleanWavs``, a
    list of paths or a text file of them), every batch mixed as ``mix_step`` mixes it with ``draw(lengths)`` -- a seeded
    ``MixDraw`` makes the pass reproducible -- peak-normalised and accumulated with ``ops.stft_stats``.  ``resample``: as
    ``CleanWavs``'s (a ``CleanWavs`` brings its own)."""
    import torch.distributed as dist
    if not isinstance(clean, CleanWavs):
        clean = CleanWavs(clean, resample)
    multi = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(), dist.get_world_size()) if multi else (0, 1)
    nfft = int(wlen_sec * fs)
    acc = ops.stats_new(nfft // 2 + 1, device)
    loader = torch.utils.data.DataLoader(torch.utils.data.Subset(clean, rank_shard(len(clean), rank, world)),
                                         batch_size=batch_size, shuffle=False, collate_fn=CleanWavs.collate)
    for batch in loader:
        lens, wave = clean_waves(batch, device)
        n = [int(v) for v in lens]
        clip, start, snr = draw(n)
        noisy = ops.mix(ops.peak_normalize(wave), n, bank, clip, start, snr)
        ops.stft_stats(acc, ops.peak_normalize(noisy), lens, nfft, int(hop_percent * nfft), eps=eps, pad_at_end=True, fs=fs)
    if multi:
        dist.all_reduce(acc)
    mean, std = ops.finalize_stats(acc)
    return Stats(audio_mean=mean.cpu().numpy().reshape(-1, 1), audio_std=std.cpu().numpy().reshape(-1, 1), eps=eps)


def read_av_files(path):
    """A text file with one "noisy clean coefficients.npy" triple of paths per line (blank lines and # comments skipped)."""
    triples = []
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].strip()
            if line:
                noisy, clean, coef = line.split()
                triples.append((noisy, clean, coef))
    return triples


class AVFiles(torch.utils.data.Dataset):
    """(noisy wav, clean wav, lip coefficients) triples: ``WavPairs`` plus the utterance's lip-region DCT coefficients, an
    ``.npy`` of shape (N, 4489) at 30 frames/s -- the matrix of NTCD-TIMIT's ``matlab_raw`` files, written with one
    ``numpy.save`` (the reference reads it from the .mat file, create_video_train_files_upsampled.py:110-112).
    ``files``: a list of triples or a text file of them.  Items: (noisy (L,), clean (L,), L, coef (N, 4489) float32)."""

    def __init__(self, files):
        self.files = read_av_files(files) if isinstance(files, str) else [tuple(p) for p in files]
        self.pairs = WavPairs([(n, c) for n, c, _ in self.files])

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        noisy, clean, n = self.pairs[i]
        coef = load_coefficients(self.files[i][2])
        return noisy, clean, n, coef

    @staticmethod
    def collate(batch):
        """-> (sample lengths (B,), noisy (B, Lmax), clean (B, Lmax), coefficient frame counts (B,), coef (sum N, 4489)):
        the waveforms zero-padded, the coefficient rows packed one utterance after the other."""
        lens, noisy, clean = WavPairs.collate([item[:3] for item in batch])
        return lens, noisy, clean, torch.LongTensor([item[3].shape[0] for item in batch]), torch.cat([item[3] for item in batch], 0)


def load_coefficients(path):
    """(N, 4489) float32 lip coefficients of one utterance from an ``.npy`` (doubles are cast, as the caller of the
    decoder must)."""
    import numpy as np
    x = np.load(path, allow_pickle=False)
    if x.ndim != 2 or x.shape[1] != ops.LIP_W * ops.LIP_H:
        raise ValueError("%s: expected (N, %d) coefficients, got shape %s" % (path, ops.LIP_W * ops.LIP_H, x.shape))
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))


def av_file_step(batch, device, labels, stats=None, acc=None, fs=16e3, wlen_sec=64e-3, hop_percent=0.25, eps=EPS, fps_in=30):
    """An ``AVFiles.collate`` batch -> (frame lengths, features (B, T, 513), video (B, T, 67, 67), target (B, T, y_dim)) on
    the GPU: ``wav_pair_step`` for the audio side and the labels, and the lip coefficients decoded and resampled to the
    STFT's frame rate (``ops.lip_decode``), capped to each utterance's label frame count and standardised with the video
    scalars of ``stats`` in the same pass.  ``acc`` (``ops.stats_new(1, device)``) collects the unstandardised frames'
    statistics.  Where the video is shorter than the labels the sequence ends with the video, as in the reference
    (create_video_train_files_upsampled.py:237-241)."""
    lens, noisy, clean, n_coef, coef = batch
    frames, x, target = wav_pair_step((lens, noisy, clean), device, labels, stats, fs, wlen_sec, hop_percent, eps)
    mean = std = None
    if stats is not None:
        mean, std = stats.get("video_mean", device), stats.get("video_std", device)
    nfft = int(wlen_sec * fs)
    video, vlen = ops.lip_decode(coef.to(device, non_blocking=True), n_coef, frames.tolist(), acc=acc, mean=mean, std=std,
                                 eps=stats.eps if stats is not None else eps, fs=int(fs), hop=int(hop_percent * nfft), fps_in=fps_in)
    T = video.shape[1]
    if T < x.shape[1]:
        x, target = x[:, :T].contiguous(), target[:, :T].contiguous()
    return vlen.to(device), x, video, target


def av_file_stats(files, device, batch_size=16, eps=EPS):
    """Train-set statistics over (noisy, clean, coefficients) triples -> ``Stats`` with the audio per-bin vectors
    (``wav_pair_stats``) and the video scalars: the decoded frames' sum / sum of squares / pixel count, accumulated in the
    pass that writes them (``ops.lip_decode(acc=...)``), each utterance capped to its label frame count -- what
    create_video_train_files_upsampled.py:294-310, 350-361 computes offline.  Ranks share the files as ``wav_pair_stats``
    does."""
    import torch.distributed as dist
    if not isinstance(files, AVFiles):
        files = AVFiles(files)
    multi = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(), dist.get_world_size()) if multi else (0, 1)
    made = wav_pair_stats(files.pairs, device, batch_size=batch_size, eps=eps)
    acc = ops.stats_new(1, device)
    loader = torch.utils.data.DataLoader(torch.utils.data.Subset(files, rank_shard(len(files), rank, world)),
                                         batch_size=batch_size, shuffle=False, collate_fn=AVFiles.collate)
    for lens, _, _, n_coef, coef in loader:
        n_label = [ops.target_frames(int(n))[1] for n in lens]
        ops.lip_decode(coef.to(device, non_blocking=True), n_coef, n_label, acc=acc)
    if multi:
        dist.all_reduce(acc)
    mean, std = ops.finalize_stats(acc)
    made._raw.update(video_mean=mean.cpu().numpy().reshape(1, 1), video_std=std.cpu().numpy().reshape(1, 1))
    return made


def forward_batch(model, kind, batch, device, waveform, stats=None, chunk_frames=None):
    """H2D, ``std_norm`` standardisation (spectrogram features and video; raw waveforms are not standardised in the
    reference either), forward.  ``chunk_frames``: evaluate through a streaming session in chunks of that many frames
    (``avvad.stream``; eval-mode models only) instead of one whole-length forward."""
    lengths = batch[0].to(device)
    data = [t.to(device, non_blocking=True) for t in batch[1:]]
    y = data[-1]
    if kind == "audio":
        x = data[0].unsqueeze(1) if waveform else (stats.audio(data[0]) if stats else data[0])
        if chunk_frames is not None:
            return lengths, stream.forward_chunked(model, x, None, lengths, chunk_frames), y
        return lengths, model(x, lengths), y
    if kind == "video":
        v = stats.video(data[0]) if stats else data[0]
        if chunk_frames is not None:
            return lengths, stream.forward_chunked(model, None, v, lengths, chunk_frames), y
        return lengths, model(v, lengths), y
    a = data[0].unsqueeze(1) if waveform else (stats.audio(data[0]) if stats else data[0])
    v = stats.video(data[1]) if stats else data[1]
    if chunk_frames is not None:
        return lengths, stream.forward_chunked(model, a, v, lengths, chunk_frames), y
    return lengths, model(a, v, lengths), y


def run_epoch(model, kind, loader, device, waveform, opt=None, reducer=None, log=None, log_interval=10, stats=None, prepare=None,
              loss_fn=None):
    """``prepare`` (wav pairs, av files): batch -> (lengths, the model's inputs ..., target) on the GPU, the model's forward
    follows.  ``loss_fn`` (logits, target, lengths) -> (loss summed over the batch, text for the log line); without one
    the summed masked BCE."""
    from packages.models.utils import batch_binary_cross_entropy, batch_f1
    train = opt is not None
    model.train(train)
    tot = dict(loss=0.0, acc=0.0, prec=0.0, rec=0.0, f1=0.0, n=0)
    for i, batch in enumerate(loader):
        if prepare is None:
            lengths, logits, y = forward_batch(model, kind, batch, device, waveform, stats)
        else:
            lengths, *x, y = prepare(batch)
            logits = model(*x, lengths)
        note = ""
        if loss_fn is None:
            loss = batch_binary_cross_entropy(logits, y, lengths, EPS)       # sum over sequences (train_AV_net.py:298-302)
        else:
            loss, note = loss_fn(logits, y, lengths)
        if train:
            loss.backward()
            if reducer is not None:
                reducer.finish()
            opt.step()
            opt.zero_grad()
        hard = (torch.sigmoid(logits.detach()) > 0.5).int()
        acc, prec, rec, f1 = batch_f1(hard, y.long(), lengths, EPS)
        for k, v in zip(("loss", "acc", "prec", "rec", "f1"), (loss.detach(), acc, prec, rec, f1)):
            tot[k] += float(v)
        tot["n"] += 1
        if log and i % log_interval == 0:
            log("%s batch %4d  loss %.3f  acc %.3f  prec %.3f  rec %.3f  f1 %.3f%s"
                % ("train" if train else "valid", i, float(loss.detach()), float(acc), float(prec), float(rec), float(f1), note))
    n = max(tot.pop("n"), 1)
    return {k: v / n for k, v in tot.items()}


def train_main(kind, make_model, model_name, waveform=False, epochs=1, batch_size=16, n_items=64, lr=1e-4,
               freeze_features=False, out_dir=None, stats=None, wav_pairs=None, compute_stats=False, av_files=None,
               objective="bce", clean_wavs=None, noise_wavs=None, snr_db=(-5.0, 20.0), mix_seed=0, mix_labels="clean",
               resample=False):
    """The body of ``scripts/train_{audio,video,AV}_net.py``; settings come from the caller's module-level constants
    (the reference's "config system") and may be overridden by AVVAD_* environment variables.

    ``wav_pairs`` (audio network, spectrogram input): a list of (noisy, clean) paths or a text file of them (``WavPairs``);
    training and validation then run on real audio, the labels computed on the GPU from the clean files -- VAD for a
    y_dim 1 head, IBM for y_dim 513 (``wav_pair_step``).  ``None`` keeps the synthetic data source.

    ``compute_stats``: with ``wav_pairs`` and no audio statistics in ``stats``, the train-set mean / std of the features
    are computed over the training pairs on the GPU before the first epoch (``wav_pair_stats``), saved under ``out_dir``
    (``Stats.save``: the directory the evaluate scripts' ``stats_dir`` takes) and used for training.

    ``av_files`` (video and AV networks, ``kind`` "video" / "AV", spectrogram input): a list of (noisy wav, clean wav,
    coefficient .npy) triples or a text file of them (``AVFiles``); the lip frames are decoded on the GPU in the step
    (``av_file_step``).  ``compute_stats`` then also fills the video scalars (``av_file_stats``).

    ``objective``: "bce" (the summed masked BCE against the labels) or, with ``wav_pairs`` and a y_dim 513 head, "si_sdr":
    minus the SI-SDR of the noisy file resynthesised through sigmoid(logits) against the clean file (``SiSdrObjective``);
    the F1 figures against the IBM label stay in the log.  Under the same conditions (``wav_pairs``, or ``clean_wavs`` with
    ``noise_wavs``; a y_dim 513 head) the mask-regression objectives of ``ops.spectral_loss`` on sigmoid(logits)
    (``SpectralObjective``): "mse_mask", the squared error against the step's label; "mse_signal", that error weighted by
    the mixture's magnitude; "msa", the complex spectrum approximation ``|S - m X|^2`` of the clean spectrum by the masked
    mixture.  And under the conditions of "si_sdr", "stoi" / "estoi": minus the summed STOI / ESTOI of the resynthesised
    wave against the clean one (``StoiObjective``, ``ops.stoi_loss``), the batch's mean score in the log line.
    Validation reports the same loss.  AVVAD_OBJECTIVE overrides it.

    ``clean_wavs`` + ``noise_wavs`` (audio network, spectrogram input, both objectives; instead of ``wav_pairs``): lists
    or text files of clean utterances (``CleanWavs``) and of noise clips (``read_noise_bank``).  Every batch is mixed on
    the GPU in the step (``mix_step``, ``ops.mix``): per row a clip, a uniform start and an SNR uniform in ``snr_db`` =
    (lo, hi) dB, drawn on the host from a generator seeded by (``mix_seed``, epoch, rank) -- a fresh draw per epoch, the
    same one in every run.  Validation draws from (``mix_seed``, "valid", rank) in every epoch, so its losses are
    comparable.  ``compute_stats`` accumulates the statistics over one pass of mixtures seeded (``mix_seed``, "stats",
    rank) (``mix_stats``).

    ``mix_labels`` (with ``clean_wavs`` + ``noise_wavs`` and a y_dim 513 head): "clean" (the default) labels the clean
    utterance alone, as wav pairs are labelled; "noise_aware" trains against the speech mask of the reference's
    ``noise_aware_IBM`` and "irm" against the ideal ratio mask, both computed in the step from the clean wave and the
    noise that was just added (``mix_step``).  With ``objective="si_sdr"`` or "msa" the label feeds the F1 log line only;
    "mse_mask" and "mse_signal" regress onto it.

    ``resample`` (with ``wav_pairs``, or ``clean_wavs`` + ``noise_wavs``): files of other rates than 16 kHz are allowed and
    resampled on the GPU -- the utterances in the step (``to_16k``), the noise clips once when the bank is read, and the
    same in the statistics passes.  The default refuses them."""
    objective = os.environ.get("AVVAD_OBJECTIVE", objective)
    check_objective(objective, kind, waveform, wav_pairs, clean_wavs=clean_wavs)
    check_mix_labels(mix_labels, clean_wavs is not None and noise_wavs is not None)
    if (clean_wavs is None) != (noise_wavs is None):
        raise ValueError("clean_wavs and noise_wavs go together: the clean utterances and the noise clips they are mixed with")
    if clean_wavs is not None:
        if wav_pairs is not None or av_files is not None:
            raise ValueError("give one data source: wav_pairs, av_files, or clean_wavs with noise_wavs")
        if kind != "audio" or waveform:
            raise ValueError("clean_wavs / noise_wavs train the audio network on spectrograms; video / AV mixing and WaveNet "
                             "waveform training on mixtures are not supported")
        snr_range(snr_db)                 # refuses a bad range before anything is set up
    if av_files is not None and (kind.lower() not in ("video", "av") or waveform or wav_pairs is not None):
        raise ValueError("av_files trains the video or the AV network on spectrograms and lip coefficients; give either "
                         "wav_pairs (audio) or av_files, and no WaveNet waveform input")
    if wav_pairs is not None and (kind != "audio" or waveform):
        raise ValueError("wav_pairs trains the audio network on spectrograms; video / AV frames and WaveNet waveform "
                         "training on wav pairs are not supported")
    epochs = int(os.environ.get("AVVAD_EPOCHS", epochs))
    n_items = int(os.environ.get("AVVAD_ITEMS", n_items))
    batch_size = int(os.environ.get("AVVAD_BATCH", batch_size))
    rank, world, local = avd.init_from_env("nccl")
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    torch.manual_seed(0)
    model = make_model().to(device)
    check_objective(objective, kind, waveform, wav_pairs, getattr(model, "y_dim", None), clean_wavs=clean_wavs)
    check_mix_labels(mix_labels, clean_wavs is not None, getattr(model, "y_dim", None))
    if freeze_features:                      # train_AV_net.py:241-245
        for name, child in model.named_children():
            if name == "features":
                for p in child.parameters():
                    p.requires_grad = False
    opt = FlatAdam(model.parameters(), lr=lr, betas=(0.9, 0.999))
    reducer = avd.BucketReducer(opt.params, opt.flat_grad, opt.offsets,
                                names=[n for n, q in model.named_parameters() if q.requires_grad]) if world > 1 else None
    prepare = loss_fn = mixer = None
    if clean_wavs is not None:
        pairs = CleanWavs(clean_wavs, resample)
        bank = read_noise_bank(noise_wavs, device, resample)
        mixer = MixDraw(bank, snr_db, mix_seed, rank)
        labels = labels_for_ydim(model.y_dim)
        collate = CleanWavs.collate
        ds_train = ds_valid = torch.utils.data.Subset(pairs, range(rank, len(pairs), world))
        prepare = lambda batch: mix_step(batch, device, labels, bank, mixer, stats, mix_labels=mix_labels)   # noqa: E731
        if objective == "si_sdr":
            step = SiSdrObjective(device, labels, lambda: stats,
                                  step=lambda batch, st: mix_step(batch, device, labels, bank, mixer, st, waves=True,
                                                                   mix_labels=mix_labels))
            prepare, loss_fn = step.prepare, step.loss
        elif objective in STOI_OBJECTIVES:
            step = StoiObjective(objective, device, labels, lambda: stats,
                                 step=lambda batch, st: mix_step(batch, device, labels, bank, mixer, st, waves=True,
                                                                  mix_labels=mix_labels))
            prepare, loss_fn = step.prepare, step.loss
        elif objective in SPECTRAL_OBJECTIVES:
            step = SpectralObjective(objective, device, labels, lambda: stats,
                                     step=lambda batch, st: mix_step(batch, device, labels, bank, mixer, st, waves=True,
                                                                      mix_labels=mix_labels, peak=True))
            prepare, loss_fn = step.prepare, step.loss
    elif av_files is not None:
        pairs = AVFiles(av_files)
        labels = labels_for_ydim(model.y_dim)
        collate = AVFiles.collate
        ds_train = ds_valid = torch.utils.data.Subset(pairs, range(rank, len(pairs), world))
        if kind.lower() == "video":
            prepare = lambda batch: (lambda r: (r[0], r[2], r[3]))(av_file_step(batch, device, labels, stats))   # noqa: E731
        else:
            prepare = lambda batch: av_file_step(batch, device, labels, stats)   # noqa: E731
    elif wav_pairs is None:
        collate = pick_collate(kind, waveform)
        per_rank = n_items // world
        ds_train = SyntheticAV(per_rank, kind, waveform=waveform, seed=1 + rank)
        ds_valid = SyntheticAV(max(per_rank // 4, batch_size), kind, waveform=waveform, seed=1000 + rank)
    else:
        pairs = WavPairs(wav_pairs, resample)
        labels = labels_for_ydim(model.y_dim)
        collate = WavPairs.collate
        ds_train = ds_valid = torch.utils.data.Subset(pairs, range(rank, len(pairs), world))
        prepare = lambda batch: wav_pair_step(batch, device, labels, stats)   # noqa: E731
        if objective == "si_sdr":
            step = SiSdrObjective(device, labels, lambda: stats)
            prepare, loss_fn = step.prepare, step.loss
        elif objective in STOI_OBJECTIVES:
            step = StoiObjective(objective, device, labels, lambda: stats)
            prepare, loss_fn = step.prepare, step.loss
        elif objective in SPECTRAL_OBJECTIVES:
            step = SpectralObjective(objective, device, labels, lambda: stats)
            prepare, loss_fn = step.prepare, step.loss
    mk = lambda ds, sh: torch.utils.data.DataLoader(ds, batch_size=batch_size // world or 1, shuffle=sh, collate_fn=collate)
    out_dir = out_dir or os.path.join("models", model_name)
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
    logf = open(os.path.join(out_dir, "output_batch.log"), "a") if rank == 0 else None

    def log(msg):
        if rank == 0:
            print(msg, flush=True)
            print(msg, file=logf, flush=True)

    from packages.utils import count_parameters
    log("- Number of learnable parameters: {}".format(count_parameters(model)))
    if compute_stats and wav_pairs is not None and (stats is None or stats.get("audio_mean", device) is None):
        t0 = time.perf_counter()
        made = wav_pair_stats(pairs, device, batch_size=batch_size)          # wav_pair_step's framing and log eps
        if stats is None:
            stats = made                    # `prepare` reads this variable when it is called
        else:
            stats._raw.update(audio_mean=made._raw["audio_mean"], audio_std=made._raw["audio_std"])
        if rank == 0:
            stats.save(out_dir)
        log("- Train-set statistics over {} pairs in {:.1f} s, saved in {}".format(len(pairs), time.perf_counter() - t0, out_dir))
    if compute_stats and clean_wavs is not None and (stats is None or stats.get("audio_mean", device) is None):
        t0 = time.perf_counter()
        made = mix_stats(pairs, bank, device, mixer.seed("stats"), batch_size=batch_size)
        if stats is None:
            stats = made
        else:
            stats._raw.update(audio_mean=made._raw["audio_mean"], audio_std=made._raw["audio_std"])
        if rank == 0:
            stats.save(out_dir)
        log("- Train-set statistics over {} mixed utterances in {:.1f} s, saved in {}".format(len(pairs), time.perf_counter() - t0, out_dir))
    if compute_stats and av_files is not None and (stats is None or stats.get("video_mean", device) is None):
        t0 = time.perf_counter()
        made = av_file_stats(pairs, device, batch_size=batch_size)
        if stats is None:
            stats = made
        else:
            stats._raw.update({k: v for k, v in made._raw.items() if stats._raw.get(k) is None})
        if rank == 0:
            stats.save(out_dir)
        log("- Train-set statistics over {} utterances in {:.1f} s, saved in {}".format(len(pairs), time.perf_counter() - t0, out_dir))
    for epoch in range(1, epochs + 1):
        t0 = time.perf_counter()
        if mixer is not None:
            mixer.seed(epoch)
        tr = run_epoch(model, kind, mk(ds_train, True), device, waveform, opt, reducer, log, stats=stats, prepare=prepare,
                       loss_fn=loss_fn)
        if mixer is not None:
            mixer.seed("valid")
        with torch.no_grad():
            va = run_epoch(model, kind, mk(ds_valid, False), device, waveform, stats=stats, prepare=prepare, loss_fn=loss_fn)
        log("====> Epoch: {:2d}  train loss {:.3f} f1 {:.3f} | valid loss {:.3f} f1 {:.3f} | {:.1f} s".format(
            epoch, tr["loss"], tr["f1"], va["loss"], va["f1"], time.perf_counter() - t0))
        if rank == 0:                       # same checkpoint naming as train_AV_net.py:443-448
            torch.save(model.state_dict(), os.path.join(out_dir, "Video_Net_epoch_{:03d}_vloss_{:.2f}.pt".format(epoch, va["loss"])))
    return model


def load_waveform(path):
    """16 kHz mono utterance as a float32 tensor: ``.wav`` (int16 PCM scaled by 1/32768 like ``torchaudio.load``) or an
    ``.npz`` holding the int16 ``samples`` of one (the committed test fixture)."""
    import numpy as np
    if path.endswith(".npz"):
        z = np.load(path, allow_pickle=False)
        x, fs = z["samples"], int(z["fs"])
    else:
        from scipy.io import wavfile
        fs, x = wavfile.read(path)
    if x.ndim > 1:
        x = x[:, 0]                      # 1 channel (evaluate_audio_net.py:120)
    if x.dtype == np.int16:
        x = x.astype(np.float32) / 32768.0
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), fs


def audio_features(x_t, stats=None, n_label_frames=None, fs=16e3, wlen_sec=64e-3, hop_percent=0.25, eps=EPS, std_norm=True):
    """``process_utt`` up to the classifier input (``evaluate_audio_net.py:122-163``) on the GPU: x / max|x| -> STFT
    (Hann 1024 / hop 256, center=False, one-hop end pad) -> re^2 + im^2 -> log(. + eps) -> crop to the label length ->
    (x - mean.T) / (std + eps).T.  Peak normalisation is its own kernel; everything behind the DFT is one epilogue pass.
    x_t (L,) on the GPU -> (1, T, 513)."""
    nfft = int(wlen_sec * fs)
    x_t = ops.peak_normalize(x_t)
    mean = std = None
    if std_norm and stats is not None:
        mean, std = stats.get("audio_mean", x_t.device), stats.get("audio_std", x_t.device)
    x = ops.stft(x_t, nfft, int(hop_percent * nfft), mode=0, eps=eps, pad_at_end=True, fs=fs, mean=mean, std=std,
                 norm_eps=stats.eps if stats is not None else eps)
    if n_label_frames is not None and n_label_frames < x.shape[1]:      # "Reduce frames of audio" (:144-146)
        x = x[:, :n_label_frames].contiguous()
    return x


def load_16k(path, device, resample=False):
    """``load_waveform`` onto the GPU at 16 kHz -> (L,): a file of another rate is resampled there (``ops.resample``) with
    ``resample``, and refused without it."""
    x, fs = load_waveform(path)
    if fs != 16000 and not resample:
        raise ValueError("%s: expected 16 kHz audio, got %d Hz" % (path, fs))
    return ops.resample(x.to(device), fs_in=fs)[0]


def clean_vad_labels(clean_path, n_noisy, device, fs=16e3, wlen_sec=64e-3, hop_percent=0.25, resample=False):
    """VAD labels (1, T) of a clean file, cropped to the noisy file's length first (the evaluator's counterpart of
    ``WavPairs``): peak normalisation, then ``clean_speech_VAD`` with the training pipeline's framing, on the GPU.
    ``resample``: a clean file of another rate is resampled to 16 kHz first (``n_noisy`` counts 16 kHz samples)."""
    c = load_16k(clean_path, device, resample)
    n = min(c.numel(), int(n_noisy))
    c = ops.peak_normalize(c[:n].to(device).view(1, -1))
    _, vad = ops.speech_targets(c, [n], "vad_labels", fs=fs, wlen_sec=wlen_sec, hop_percent=hop_percent, center=False,
                                pad_at_end=True)
    return vad.view(1, -1)


def _one_chunking(chunk_frames, chunk_samples):
    if chunk_frames is not None and chunk_samples is not None:
        raise ValueError("chunk_frames (features in, frames per step) and chunk_samples (samples in) exclude each other")


def process_utt(classifier, x_t, stats=None, n_label_frames=None, video=None, eps=EPS, std_norm=True, chunk_frames=None,
                chunk_samples=None, fs_in=16000):
    """One utterance through the reference's evaluator (``evaluate_audio_net.py:107-180``; with ``video`` (T,67,67) the AV
    variant ``evaluate_AV_net.py:148-250``): returns (y_hat_soft, y_hat_hard) on the CPU, shaped (1, T) like the
    reference's ``y_hat_soft[..., 0]``.  ``chunk_frames``: score through a streaming session (``avvad.stream``), that
    many frames per step; the features are still formed from the whole utterance.  ``chunk_samples``: the RAW samples go
    through the session in packets of that many (``stream.forward_wave_chunked``): the peak -- the one statistic of the
    whole utterance -- is one reduction up front, everything behind it is streamed.  ``fs_in``: the rate of ``x_t``; another
    rate than 16000 is resampled on the GPU first (``ops.resample``), and with ``chunk_samples`` the packets are taken at
    ``fs_in`` and resampled inside the session."""
    soft = torch.sigmoid(utt_logits(classifier, x_t, stats, n_label_frames, video, eps, std_norm, chunk_frames,
                                    chunk_samples, fs_in)[..., 0].detach().cpu())
    return soft, (soft > 0.5).int()


def utt_logits(classifier, x_t, stats=None, n_label_frames=None, video=None, eps=EPS, std_norm=True, chunk_frames=None,
               chunk_samples=None, fs_in=16000):
    """The logits (1, T, y_dim) of ``process_utt``, on the GPU (arguments as there)."""
    _one_chunking(chunk_frames, chunk_samples)
    x16 = ops.resample(x_t.reshape(-1), fs_in=fs_in)[0]          # x_t itself at 16 kHz
    if chunk_samples is not None:
        w = x_t.reshape(1, -1)
        T = ops.n_frames(x16.numel(), 1024, 256)
        T = T if n_label_frames is None else min(T, int(n_label_frames))
        v = None
        if video is not None:
            v = video[None, :T].contiguous()
            v = stats.video(v) if (stats is not None and std_norm) else v
        return stream.forward_wave_chunked(classifier, w, None, v, chunk_samples, stats if std_norm else None,
                                           ops.peak(x16.view(1, -1)), eps=eps, max_frames=[T], fs_in=fs_in)
    x = audio_features(x16, stats, n_label_frames, eps=eps, std_norm=std_norm)
    lengths = [x.shape[1]]
    v = None
    if video is not None:
        v = video[None, :x.shape[1]].contiguous()
        v = stats.video(v) if (stats is not None and std_norm) else v
    if chunk_frames is not None:
        y = stream.forward_chunked(classifier, x, v, lengths, chunk_frames)
    elif video is None:
        y = classifier(x, lengths)
    else:
        y = classifier(x, v, lengths)
    return y


def resynth_utt(classifier, x_t, stats=None, hard=True, eps=EPS, std_norm=True, chunk_samples=None, fs_in=16000):
    """Enhanced waveform of one utterance from a mask-predicting audio model (``y_dim = n_fft/2 + 1 = 513``): peak
    normalisation -> features -> model as in ``process_utt``, then the logits go straight in as the mask of
    ``ops.resynth`` on the peak-normalised wave -- ``hard``: ``logit > 0`` (the evaluator's ``sigmoid > 0.5``), else
    ``sigmoid(logit)`` -- with the peak as the output scale, so the result is in the input's scale.  x_t (L,) on the GPU
    -> (L,) on the GPU.  ``chunk_samples``: the raw samples go through a streaming session in packets of that many and the
    enhanced samples come out of it per packet (``stream.enhance_wave_chunked``) -- the same values up to summation order
    (with ``hard``, a logit next to 0 may fall on the other side).  ``fs_in``: the rate of ``x_t``; the enhanced samples
    are 16 kHz, ``ops.resample_length(L)`` of them (resampling back is out of scope)."""
    n_fft = 1024
    if getattr(classifier, "y_dim", None) != n_fft // 2 + 1:
        raise ValueError("resynthesis needs a model that predicts a %d-bin mask (y_dim = %d), got y_dim = %r"
                         % (n_fft // 2 + 1, n_fft // 2 + 1, getattr(classifier, "y_dim", None)))
    x16 = ops.resample(x_t.reshape(-1), fs_in=fs_in)[0]
    if chunk_samples is not None:
        return stream.enhance_wave_chunked(classifier, x_t.reshape(1, -1), None, chunk_samples, stats if std_norm else None,
                                           ops.peak(x16.view(1, -1)), hard, eps, n_fft, 256, fs_in).view(-1)
    w = x16.view(1, -1)
    x = audio_features(x16, stats, None, eps=eps, std_norm=std_norm)
    logits = classifier(x, [x.shape[1]]).detach().contiguous()
    out = ops.resynth(ops.peak_normalize(w), logits, mask_mode=3 if hard else 2, n_fft=n_fft, hop=256, scale=ops.peak(w))
    return out.view(-1)


def score_utt(enhanced, clean, noisy):
    """Enhancement scores of one utterance on the GPU: a dict of Python floats ``si_sdr``, ``si_sir``, ``si_sar`` (the
    enhanced signal against the clean one, the noise being ``noisy - clean``) and ``input_si_sdr`` (the noisy signal
    itself against the clean one).  One two-row ``ops.energy_ratios`` call: rows ``enhanced`` and ``noisy``, both scored
    against ``clean`` with ``mixture = noisy``.  The three (L,) GPU signals are cropped to their common length."""
    n = min(enhanced.numel(), clean.numel(), noisy.numel())
    e, c, x = (t.reshape(-1)[:n] for t in (enhanced, clean, noisy))
    r = ops.energy_ratios(torch.stack([e, x]), torch.stack([c, c]), mixture=torch.stack([x, x])).tolist()
    return {"si_sdr": r[0][0], "si_sir": r[0][1], "si_sar": r[0][2], "input_si_sdr": r[1][0]}


SCORE_KEYS = ("si_sdr", "si_sir", "si_sar", "input_si_sdr")
INTELLIGIBILITY_KEYS = ("stoi", "estoi", "input_stoi", "input_estoi")


def intelligibility_utt(enhanced, clean, noisy):
    """Intelligibility scores of one 16 kHz utterance on the GPU: a dict of Python floats ``stoi``, ``estoi`` (the enhanced
    signal against the clean one) and ``input_stoi``, ``input_estoi`` (the noisy signal itself).  One two-row ``ops.stoi``
    call: rows ``enhanced`` and ``noisy`` against the same ``clean``.  The three (L,) GPU signals are cropped to their
    common length."""
    n = min(enhanced.numel(), clean.numel(), noisy.numel())
    e, c, x = (t.reshape(-1)[:n] for t in (enhanced, clean, noisy))
    d = ops.stoi(torch.stack([c, c]), torch.stack([e, x]), fs=16000, both=True).tolist()
    return {"stoi": d[0][0], "estoi": d[0][1], "input_stoi": d[1][0], "input_estoi": d[1][1]}


def evaluate_main(kind, make_model, checkpoint=None, waveform=False, n_items=16, out_dir="eval_out", wav_list=None,
                  stats=None, labels=None, clean_of=None, av_files=None, chunk_frames=None, chunk_samples=None,
                  resynth_dir=None, resynth_hard=True, resynth_chunked=False, score_dir=None,
                  intelligibility=False, resample=False):
    """The body of ``scripts/evaluate_*_net.py``: per-utterance forward, sigmoid, threshold, save
    ``*_y_hat_soft.pt`` / ``*_y_hat_hard.pt`` (``evaluate_AV_net.py:236-250``); utterances are split across ranks
    (the reference's 4-process pool, ``:329-339``).

    ``wav_list`` (audio network): paths of 16 kHz utterances (.wav / .npz) that go through ``process_utt`` -- the
    reference's plumbing on real audio; ``labels`` optionally maps a path to its label tensor (frame count crop + saved
    next to the predictions for ``run_metrics``).  ``clean_of`` maps each noisy path of ``wav_list`` to its clean
    counterpart: the labels are then the clean file's VAD (peak-normalised, the training pipeline's framing), computed on
    the GPU, in place of ``labels``.  ``av_files`` (video and AV networks): (noisy wav, clean wav, coefficient .npy)
    triples or a text file of them; every utterance goes through ``av_file_step`` on its own -- features and decoded lip
    frames standardised with ``stats``, the clean file's VAD as the label.  Without either a synthetic ragged data
    source stands in for the HDF5 datasets.  ``chunk_frames``: every utterance is scored through a streaming session
    (``avvad.stream``) in chunks of that many frames -- same files, same values up to summation order; ``None`` is the
    whole-length forward.  ``chunk_samples`` (``wav_list``, and ``av_files`` with the AV network): every utterance's raw
    samples are streamed in packets of that many, the STFT front-end included (``process_utt``); for ``av_files`` the
    whole-utterance step still runs first, for the labels, the decoded lip frames and the frame count, and its audio
    features are not used.

    ``resynth_dir`` (``wav_list`` with a 513-output audio model): every utterance is also resynthesised from the model's
    mask (``resynth_utt``; ``resynth_hard``: binary mask, else the soft one) and written there as ``<base>_enhanced.wav``
    -- float32, 16 kHz, as many samples as the input.  ``None`` writes nothing.  ``resynth_chunked`` (with ``resynth_dir``
    and ``chunk_samples``): the enhanced samples come out of the streaming session, packet by packet.

    ``score_dir`` (``wav_list`` with ``clean_of``): every utterance is scored on the GPU and ``<base>_scores.pt`` is
    written there, a dict of Python numbers: the classifier's ``tp, tn, fp, fn`` (``ops.confusion_counts`` on the logits
    the predictions come from and the GPU labels) and, with ``resynth_dir``, ``score_utt`` of the enhanced waveform
    against the clean file cropped to the common length.  ``None`` writes nothing and changes nothing.
    ``intelligibility`` (with ``resynth_dir`` and ``score_dir``): ``intelligibility_utt``'s four keys ``stoi``, ``estoi``,
    ``input_stoi``, ``input_estoi`` join that dict; ``False`` leaves the file exactly as it was.

    ``resample`` (``wav_list``): an utterance (or its clean file) of another rate than 16 kHz is resampled on the GPU
    (``ops.resample``) and then scored as a 16 kHz one -- predictions, labels, ``resynth_dir`` and ``score_dir`` outputs are
    all 16 kHz; with ``chunk_samples`` the packets are taken at the file's rate and resampled inside the session
    (``Session.set_frontend(fs_in=...)``).  The default refuses such a file."""
    if intelligibility and (resynth_dir is None or score_dir is None):
        raise ValueError("intelligibility scores the enhanced utterances: it needs resynth_dir and score_dir")
    if score_dir is not None and (wav_list is None or clean_of is None):
        raise ValueError("score_dir scores the utterances of wav_list against their clean files: it needs clean_of")
    _one_chunking(chunk_frames, chunk_samples)
    if resynth_chunked and (resynth_dir is None or chunk_samples is None):
        raise ValueError("resynth_chunked streams the resynthesis: it needs resynth_dir and chunk_samples")
    model = None
    if resynth_dir is not None:
        if wav_list is None or kind != "audio":
            raise ValueError("resynth_dir writes the enhanced utterances of wav_list for the audio network")
        torch.manual_seed(0)
        model = make_model()
        if getattr(model, "y_dim", None) != 513:
            raise ValueError("resynth_dir needs a model that predicts a 513-bin mask (y_dim = 513), got y_dim = %r"
                             % (getattr(model, "y_dim", None),))
    if chunk_samples is not None and (wav_list is None and av_files is None or kind.lower() == "video"):
        raise ValueError("chunk_samples streams the waveform of wav_list / av_files utterances into an audio or AV network")
    rank, world, local = avd.init_from_env("nccl")
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    torch.manual_seed(0)
    if model is None:
        model = make_model()
    if checkpoint:
        model.load_state_dict(torch.load(checkpoint, map_location="cpu", weights_only=True))
    model = model.to(device).eval()
    for p in model.parameters():
        p.requires_grad = False
    os.makedirs(out_dir, exist_ok=True)
    if resynth_dir is not None:
        os.makedirs(resynth_dir, exist_ok=True)
    if score_dir is not None:
        os.makedirs(score_dir, exist_ok=True)
    t0 = time.perf_counter()
    if av_files is not None:
        if kind.lower() not in ("video", "av") or waveform or wav_list is not None:
            raise ValueError("av_files drives the video and AV evaluators on spectrograms; wav_list is the audio evaluator's")
        files = AVFiles(av_files)
        with torch.no_grad():
            for i in range(rank, len(files), world):
                batch = AVFiles.collate([files[i]])
                lengths, x, video, y = av_file_step(batch, device, "vad_labels", stats)
                if chunk_samples is not None:
                    w = batch[1].to(device)
                    logits = stream.forward_wave_chunked(model, w, None, video, chunk_samples, stats, ops.peak(w),
                                                         max_frames=lengths.tolist())
                elif chunk_frames is not None:
                    logits = stream.forward_chunked(model, None if kind.lower() == "video" else x, video, lengths, chunk_frames)
                else:
                    logits = model(video, lengths) if kind.lower() == "video" else model(x, video, lengths)
                soft = torch.sigmoid(logits[..., 0].detach().cpu())
                base = os.path.join(out_dir, os.path.splitext(os.path.basename(files.files[i][0]))[0])
                torch.save((soft > 0.5).int(), base + "_y_hat_hard.pt")
                torch.save(soft, base + "_y_hat_soft.pt")
                torch.save(y[:, :int(lengths[0]), 0].int().cpu(), base + "_label.pt")
    elif wav_list is not None:
        if kind != "audio":
            raise ValueError("wav_list drives the audio evaluator (evaluate_audio_net.py); video needs the HDF5 readers")
        with torch.no_grad():
            for i in range(rank, len(wav_list), world):
                x_t, fs = load_waveform(wav_list[i])
                if fs != 16000 and not resample:
                    raise ValueError("%s: expected 16 kHz audio, got %d Hz" % (wav_list[i], fs))
                x_in = x_t.to(device)                             # as read, at the file's rate: what the packets are cut from
                x_t = ops.resample(x_in, fs_in=fs)[0]             # at 16 kHz (the tensor itself when it is)
                if clean_of is not None:
                    y = clean_vad_labels(clean_of[wav_list[i]], x_t.numel(), device, resample=resample)
                else:
                    y = labels.get(wav_list[i]) if labels else None
                logits = utt_logits(model, x_in, stats, None if y is None else y.shape[-1],
                                    chunk_frames=chunk_frames, chunk_samples=chunk_samples, fs_in=fs)
                soft = torch.sigmoid(logits[..., 0].detach().cpu())                      # process_utt's outputs
                hard = (soft > 0.5).int()
                scores = None
                if score_dir is not None:
                    Tn = min(logits.shape[1], y.shape[-1])
                    counts = ops.confusion_counts(logits[:, :Tn, 0].detach().contiguous(), y[:, :Tn].float().contiguous(),
                                                  logits=True)[0].tolist()
                    scores = dict(zip(("tp", "tn", "fp", "fn"), counts))
                base = os.path.join(out_dir, os.path.splitext(os.path.basename(wav_list[i]))[0])
                torch.save(hard, base + "_y_hat_hard.pt")
                torch.save(soft, base + "_y_hat_soft.pt")
                if y is not None:
                    torch.save(y.int().cpu(), base + "_label.pt")
                if resynth_dir is not None:
                    from scipy.io import wavfile
                    enhanced = resynth_utt(model, x_in, stats, hard=resynth_hard,
                                           chunk_samples=chunk_samples if resynth_chunked else None, fs_in=fs)
                    wavfile.write(os.path.join(resynth_dir, os.path.basename(base) + "_enhanced.wav"), 16000,
                                  enhanced.cpu().numpy())
                    if scores is not None:
                        clean = load_16k(clean_of[wav_list[i]], device, resample)
                        scores.update(score_utt(enhanced, clean, x_t))
                        if intelligibility:
                            scores.update(intelligibility_utt(enhanced, clean, x_t))
                if scores is not None:
                    torch.save(scores, os.path.join(score_dir, os.path.basename(base) + "_scores.pt"))
    else:
        ds = SyntheticAV(n_items, kind, waveform=waveform, seed=7)
        collate = pick_collate(kind, waveform)
        with torch.no_grad():
            for i in range(rank, n_items, world):
                batch = collate([ds[i]])
                lengths, logits, y = forward_batch(model, kind, batch, device, waveform, stats, chunk_frames)
                soft = torch.sigmoid(logits[..., 0].detach().cpu())                      # (1,T), evaluate_AV_net.py:236-240
                torch.save(soft, os.path.join(out_dir, "utt%04d_y_hat_soft.pt" % i))
                torch.save((soft > 0.5).int(), os.path.join(out_dir, "utt%04d_y_hat_hard.pt" % i))
                torch.save(y[..., 0].int().cpu(), os.path.join(out_dir, "utt%04d_label.pt" % i))   # synthetic stand-in for the labels
    if rank == 0:
        print("Finished in {:.2f} seconds".format(time.perf_counter() - t0))


def metrics_main(out_dir="eval_out", confidence=0.95, eps=1e-8, score_dir=None, intelligibility=False):
    """The body of ``scripts/run_metrics_dnn_classif.py`` (``:102-300``) for the classifier outputs: per utterance
    ``f1_loss(y_hat_hard, y)`` -> (accuracy, precision, recall, F1), then ``compute_stats`` tables with Student-t
    confidence intervals.  Reads the ``*_y_hat_hard.pt`` / ``*_label.pt`` pairs that ``evaluate_main`` wrote.
    ``score_dir``: a second table over the four enhancement scores of the ``*_scores.pt`` files that
    ``evaluate_main(resynth_dir=..., score_dir=...)`` wrote there; both tables are then returned as
    ``{"classifier": ..., "enhancement": ...}``.  ``intelligibility``: the enhancement table also holds the four
    ``INTELLIGIBILITY_KEYS`` that ``evaluate_main(..., intelligibility=True)`` wrote."""
    import glob
    from packages.metrics import compute_stats
    from packages.models.utils import f1_loss
    rows = []
    for hard_path in sorted(glob.glob(os.path.join(out_dir, "*_y_hat_hard.pt"))):
        y_hat = torch.load(hard_path, weights_only=True).reshape(-1)
        y = torch.load(hard_path.replace("_y_hat_hard.pt", "_label.pt"), weights_only=True).reshape(-1)
        rows.append(tuple(float(v) for v in f1_loss(y_hat, y.long(), eps)))
    if len(rows) < 2:
        raise SystemExit("need at least two evaluated utterances in %s (run scripts/evaluate_*_net.py first)" % out_dir)
    table = compute_stats(metrics_keys=["accuracy", "precision", "recall", "f1score"], all_metrics=rows, model_data_dir=out_dir,
                          confidence=confidence)
    if score_dir is None:
        return table
    scored = [torch.load(path, weights_only=True) for path in sorted(glob.glob(os.path.join(score_dir, "*_scores.pt")))]
    keys = SCORE_KEYS + (INTELLIGIBILITY_KEYS if intelligibility else ())
    scored = [tuple(d[k] for k in keys) for d in scored if all(k in d for k in keys)]
    if len(scored) < 2:
        raise SystemExit("need at least two scored utterances in %s (evaluate_main with resynth_dir and score_dir)" % score_dir)
    return {"classifier": table, "enhancement": compute_stats(metrics_keys=list(keys), all_metrics=scored,
                                                              model_data_dir=score_dir, confidence=confidence)}
