"""Training entry point with the settings block of the reference's ``scripts/train_AV_net.py`` (module-level
constants are the configuration, as there).  Run from the package root -- ``python scripts/train_AV_net.py`` -- or one
process per GPU under ``python -m torch.distributed.run --nproc-per-node N scripts/train_AV_net.py``, which replaces
the reference's ``nn.DataParallel(model, device_ids=[0,1,2,3])`` by bucketed RCCL all-reduce.
Inputs: spectrogram features + lip crops; ``use_mcb`` selects compact bilinear fusion (the reference's default, :70) or concat;
``freeze_resnet`` reproduces the frozen trunk of train_AV_net.py:241-245.
The loop body (standardise -> forward -> summed masked BCE -> backward -> Adam -> per-sequence F1 -> checkpoint
``Video_Net_epoch_XXX_vloss_Y.pt``) is ``avvad.train.train_main``; a synthetic ragged data source stands in for the
reference's HDF5 datasets (h5py is not installed in this image).  AVVAD_EPOCHS / AVVAD_ITEMS / AVVAD_BATCH override sizes."""
import sys
sys.path.append('.')

from avvad.train import Stats, train_main
from packages.models.AV_Net import DeepVAD_AV

# Settings (names as in the reference script)
lstm_layers = 2
lstm_hidden_size = 1024
y_dim = 1                 # 1: VAD labels; 513: IBM labels (train_AV_net.py:64-66)
batch_size = 16
learning_rate = 1e-4
end_epoch = 1
eps = 1e-8
std_norm = True           # standardise inputs with the train-set statistics when models/<model_name>/trainset_*.npy exist
model_name = 'AV_Classif_synthetic'
av_files = None           # text file with one "noisy.wav clean.wav lips.npy" triple per line: train on real data, the lip
                          # coefficients ((N, 4489) at 30 frames/s) decoded on the GPU, labels from the clean files; None: synthetic
compute_stats = False     # with av_files and no trainset_*.npy yet: compute the train-set statistics (audio per bin, video
                          # scalars) on the GPU before the first epoch and save them in models/<model_name>
use_mcb = True
freeze_resnet = False
WAVENET = False           # True: raw waveforms through the WaveNet encoder (the hook the reference left commented out)
wavenet_params = dict(filter_width=2, quantization_channel=1, dilations=[2 ** i for i in range(10)] * 2,
                      en_residual_channel=32, en_dilation_channel=32, en_bottleneck_width=256,
                      en_pool_kernel_size=16, use_bias=True)


def make_model():
    return DeepVAD_AV(lstm_layers, lstm_hidden_size, y_dim, use_mcb=use_mcb, eps=eps, wavenet_params=wavenet_params if WAVENET else None)


if __name__ == '__main__':
    stats = Stats.load('models/' + model_name, eps) if std_norm else None
    train_main('av', make_model, model_name, waveform=WAVENET, epochs=end_epoch, batch_size=batch_size,
               lr=learning_rate, stats=stats, freeze_features=freeze_resnet, av_files=av_files,
               compute_stats=compute_stats and std_norm)
