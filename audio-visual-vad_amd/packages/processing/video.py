"""Counterpart of the reference's ``packages/processing/video.py`` (``preprocess_ntcd_matlab``: one frame of NTCD-TIMIT's
lip-region DCT coefficients -> inverse DCT -> rotated image) for whole utterances, computed by the HIP kernels of
``csrc/lip.hip``: ``decode_ntcd_frames`` is the frame pipeline of ``scripts/create_video_train_files_upsampled.py:105-173``
-- 2-D inverse DCT, normalisation over the utterance, ``rot90(., 3)``, 8-bit quantisation, resampling from 30 frames/s to
the STFT's frame rate.  The reference's per-frame normalisation (``preprocess_ntcd_matlab`` scales every frame by its own
range) is the visualisation path and is not ported; the codec round trip of the training files is not modelled.

A numpy array or a CPU tensor is moved to the GPU, decoded there and returned as a float32 numpy array; a GPU tensor gives
a GPU tensor.  This is not a CPU fallback: without a GPU the function raises ``AvvadError``."""
import numpy as np
import torch


def decode_ntcd_frames(matlab_frames, n_label_frames=None, width=67, height=67, visual_frame_rate_i=30, fs=16000, hop=256,
                       quantize=True, device=None):
    """``matlab_frames`` (N, width*height): the coefficient rows of one utterance as the ``.mat`` files hold them (doubles
    are cast to float32).  Returns the video (T, height, width), T = ``ops.lip_out_frames(N)`` capped by
    ``n_label_frames`` -- the layout ``process_utt(video=...)`` and the video network take."""
    from avvad import ops
    from avvad._lib import AvvadError
    if (width, height) != (ops.LIP_W, ops.LIP_H):
        raise AvvadError("the lip decoder is built for %dx%d frames, got %dx%d" % (ops.LIP_W, ops.LIP_H, width, height))
    host = not (isinstance(matlab_frames, torch.Tensor) and matlab_frames.is_cuda)
    if host:
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise AvvadError("decode_ntcd_frames: the lip decoder runs on the GPU -- there is no CPU fallback")
        t = matlab_frames if isinstance(matlab_frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(matlab_frames))
        x = t.to(dev)
    else:
        x = matlab_frames
    x = x.float().reshape(-1, width * height).contiguous()
    video, _ = ops.lip_decode(x, [x.shape[0]], None if n_label_frames is None else [int(n_label_frames)], quantize=quantize,
                              fs=fs, hop=hop, fps_in=visual_frame_rate_i)
    return video[0].cpu().numpy() if host else video[0]
