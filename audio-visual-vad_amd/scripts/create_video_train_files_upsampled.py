"""What is left of the reference's ``scripts/create_video_train_files_upsampled.py`` here: the train-set statistics.  The
reference script decodes the lip-region DCT coefficients of every utterance (inverse DCT, normalisation, rotation, ffmpeg
resampling to the STFT's frame rate), writes the frames and labels into HDF5 and accumulates the scalar pixel mean / std
(lines 105-173, 294-310, 350-361).  In this port the frames and the labels are computed in the training step from the wav
files and the coefficient matrices themselves (``avvad.train.av_file_step``, ``ops.lip_decode``), so the only product
still needed ahead of training is ``trainset_{audio,video}_{mean,std}.npy`` -- a list of (noisy wav, clean wav,
coefficient .npy) triples in, the four float32 files out, reduced on the GPU in the pass that decodes the frames
(``avvad.train.av_file_stats``).  A coefficient file is the (N, 4489) matrix of an utterance's ``matlab_raw`` .mat file
written with ``numpy.save``.  Run from the package root -- ``python scripts/create_video_train_files_upsampled.py`` -- or
one process per GPU under ``python -m torch.distributed.run``.  ``scripts/train_video_net.py`` / ``train_AV_net.py`` with
``compute_stats = True`` do the same before their first epoch."""
import sys
sys.path.append('.')

import time

import torch

from avvad import dist as avd
from avvad.train import av_file_stats

# Parameters (names as in the reference script)
## Dataset
av_files = None           # text file with one "noisy.wav clean.wav lips.npy" triple per line: the TRAIN split
batch_size = 16           # utterances per decode call

## Video
visual_frame_rate_i = 30  # frames/s of the coefficient files; the output rate is the STFT's, fs / hop = 62.5 frames/s
width = 67
height = 67
eps = 1e-8

## Output
model_name = 'video_Classif_synthetic'
output_dir = 'models/' + model_name      # where scripts/train_video_net.py and the evaluate scripts' stats_dir look


if __name__ == '__main__':
    if av_files is None:
        raise SystemExit("set av_files to a text file with one 'noisy.wav clean.wav lips.npy' triple per line")
    rank, world, local = avd.init_from_env("nccl")
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    t1 = time.perf_counter()
    stats = av_file_stats(av_files, device, batch_size=batch_size, eps=eps)
    if rank == 0:
        stats.save(output_dir)
        print(f'Finished in {time.perf_counter() - t1} seconds')
        print('Mean and std saved in ' + output_dir)
