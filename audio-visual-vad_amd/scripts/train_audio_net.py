"""Training entry point with the settings block of the reference's ``scripts/train_audio_net.py`` (module-level
constants are the configuration, as there).  Run from the package root -- ``python scripts/train_audio_net.py`` -- or one
process per GPU under ``python -m torch.distributed.run --nproc-per-node N scripts/train_audio_net.py``, which replaces
the reference's ``nn.DataParallel(model, device_ids=[0,1,2,3])`` by bucketed RCCL all-reduce.
Inputs: 513-bin log-power spectrogram sequences (B,T,513) or, with WAVENET = True, raw waveforms through the WaveNet encoder.
The loop body (standardise -> forward -> summed masked BCE -> backward -> Adam -> per-sequence F1 -> checkpoint
``Video_Net_epoch_XXX_vloss_Y.pt``) is ``avvad.train.train_main``; with ``wav_pairs`` it trains on (noisy, clean) wav pairs
and computes the labels on the GPU, otherwise a synthetic ragged data source stands in for the reference's HDF5
datasets (h5py is not installed in this image).  With ``objective = 'si_sdr'`` (wav pairs, y_dim 513) the loss is the
SI-SDR of the waveform resynthesised through the sigmoid mask instead of the BCE against the IBM label.
AVVAD_EPOCHS / AVVAD_ITEMS / AVVAD_BATCH override sizes, AVVAD_OBJECTIVE the objective."""
import sys
sys.path.append('.')

from avvad.train import Stats, train_main
from packages.models.Audio_Net import DeepVAD_audio

# Settings (names as in the reference script)
lstm_layers = 2
lstm_hidden_size = 1024
y_dim = 1                 # 1: VAD labels; 513: IBM labels (train_AV_net.py:64-66)
batch_size = 16
learning_rate = 1e-4
end_epoch = 1
eps = 1e-8
std_norm = True           # standardise inputs with the train-set statistics when models/<model_name>/trainset_*.npy exist
model_name = 'audio_Classif_synthetic'
WAVENET = False           # True: raw waveforms through the WaveNet encoder (the hook the reference left commented out)
wav_pairs = None          # text file with one "noisy.wav clean.wav" pair per line: train on real audio, labels computed on
                          # the GPU from the clean files (VAD for y_dim 1, IBM for y_dim 513); None: synthetic data
compute_stats = False     # with wav_pairs and no trainset_audio_*.npy yet: compute the train-set mean / std over the pairs on
                          # the GPU before the first epoch and save them in models/<model_name> (the evaluate scripts' stats_dir)
objective = 'bce'         # 'si_sdr' (wav_pairs, y_dim 513): minus the SI-SDR of the noisy file resynthesised through the
                          # sigmoid of the logits, against the clean file; the F1 figures against the IBM stay in the log.
                          # 'mse_mask' | 'mse_signal' | 'msa' (same conditions): the mask-regression losses on the sigmoid of
                          # the logits -- squared error against the label, that error weighted by the mixture's magnitude,
                          # the complex spectrum approximation |S - m X|^2 (avvad.train.SpectralObjective)
wavenet_params = dict(filter_width=2, quantization_channel=1, dilations=[2 ** i for i in range(10)] * 2,
                      en_residual_channel=32, en_dilation_channel=32, en_bottleneck_width=256,
                      en_pool_kernel_size=16, use_bias=True)


def make_model():
    return DeepVAD_audio(lstm_layers, lstm_hidden_size, y_dim, wavenet_params=wavenet_params if WAVENET else None)


if __name__ == '__main__':
    stats = Stats.load('models/' + model_name, eps) if std_norm else None
    train_main('audio', make_model, model_name, waveform=WAVENET, epochs=end_epoch, batch_size=batch_size,
               lr=learning_rate, stats=stats, wav_pairs=wav_pairs, compute_stats=compute_stats and std_norm,
               objective=objective)
