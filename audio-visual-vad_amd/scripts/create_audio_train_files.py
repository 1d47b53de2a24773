"""What is left of the reference's ``scripts/create_audio_train_files.py`` here: the train-set statistics.  The reference
script writes spectrograms, labels and the per-bin mean / std of the log-power spectrogram into HDF5; in this port the
spectrogram and the labels are computed in the training step from the wav files themselves (``avvad.train.wav_pair_step``),
so the only product still needed ahead of training is ``trainset_audio_{mean,std}.npy`` -- a list of (noisy, clean) wav
pairs in, the two (513, 1) float32 files out, reduced on the GPU (``avvad.train.wav_pair_stats``: per-bin sum, sum of
squares and count in double over every frame of the set, ``mean = sum / n``, ``std = sqrt((sumsq - n mean^2) / (n - 1))``,
the formula of lines 196-214 and 340-392 of the reference script).  Run from the package root --
``python scripts/create_audio_train_files.py`` -- or one process per GPU under ``python -m torch.distributed.run``: every
rank reduces its share of the pairs and the accumulators are summed before the division.  ``scripts/train_audio_net.py``
with ``compute_stats = True`` does the same before its first epoch."""
import sys
sys.path.append('.')

import time

import torch

from avvad import dist as avd
from avvad.train import wav_pair_stats

# Parameters (names as in the reference script)
## Dataset
wav_pairs = None          # text file with one "noisy.wav clean.wav" pair per line: the TRAIN split
batch_size = 16           # utterances per reduction call

## STFT
fs = int(16e3)            # Sampling rate
wlen_sec = 64e-3          # window length in seconds
hop_percent = 0.25        # hop size as a percentage of the window length
center = False
pad_at_end = True         # pad audio file at end to match same size after stft + istft
eps = 1e-8                # log(|X|^2 + eps)

## Output
model_name = 'audio_Classif_synthetic'
output_dir = 'models/' + model_name      # where scripts/train_audio_net.py and the evaluate scripts' stats_dir look


if __name__ == '__main__':
    if wav_pairs is None:
        raise SystemExit("set wav_pairs to a text file with one 'noisy.wav clean.wav' pair per line")
    rank, world, local = avd.init_from_env("nccl")
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    t1 = time.perf_counter()
    stats = wav_pair_stats(wav_pairs, device, batch_size=batch_size, fs=fs, wlen_sec=wlen_sec, hop_percent=hop_percent, eps=eps)
    if rank == 0:
        stats.save(output_dir)
        print(f'Finished in {time.perf_counter() - t1} seconds')
        print('Mean and std saved in ' + output_dir)
