"""Drop-in containers for ``packages/models/compact_bilinear_pooling.py`` (``CountSketch`` ``:59-114``,
``CompactBilinearPooling`` ``:222-263``): same constructor arguments, buffers ``h`` (int64 bucket of each
input channel) / ``s`` (+-1 sign) and sub-module names ``sketch1`` / ``sketch2`` so MCB checkpoints load.
``forward`` of both modules runs the stand-alone HIP kernels (``avvad_count_sketch_fwd/bwd``,
``avvad_mcb_fwd/bwd``: csrc/mcb.hip -- the FFT product of the reference is evaluated as the circular
convolution it equals) and returns the raw sketch / pooled vector like the reference; inside ``DeepVAD_AV``
the same arithmetic runs fused with the signed sqrt, L2 norm and BatchNorm1d (``ops.McbFusionFn``).
GPU tensors only: there is no PyTorch fallback.
The kernels index with ``h`` unchecked (a global read at ``dout[row * D + h[c]]``, an LDS index ``D - h``), and a buffer
comes from wherever a checkpoint comes from: ``CountSketch`` validates it on the host where it receives it -- the
constructor and ``load_state_dict`` -- and ``forward`` stays free of any device synchronisation."""
import torch
import torch.nn as nn

from avvad import AvvadError, ops


def _check_hashes(h, input_size, output_size, name="h"):
    """int64, shape (input_size,), every value in [0, output_size): or AvvadError"""
    if not isinstance(h, torch.Tensor) or h.dtype != torch.long:
        raise AvvadError("%s must be an int64 tensor, got %s" % (name, h.dtype if isinstance(h, torch.Tensor) else type(h).__name__))
    if tuple(h.shape) != (input_size,):
        raise AvvadError("%s must have shape (%d,), got %s" % (name, input_size, tuple(h.shape)))
    if input_size and (int(h.min()) < 0 or int(h.max()) >= output_size):
        raise AvvadError("%s must lie in [0, %d): found values from %d to %d" % (name, output_size, int(h.min()), int(h.max())))


class CountSketch(nn.Module):
    def __init__(self, input_size, output_size, h=None, s=None):
        super().__init__()
        self.input_size = input_size
        self.output_size = output_size
        if h is None:
            h = torch.randint(0, output_size, (input_size,), dtype=torch.long)
        if s is None:
            s = 2.0 * torch.randint(0, 2, (input_size,)).float() - 1.0
        _check_hashes(h, input_size, output_size)
        self.register_buffer("h", h)
        self.register_buffer("s", s)

    def _apply(self, fn, recurse=True):
        # `h` must stay int64 whatever dtype the module is cast to (reference :96-104)
        h = self.h
        super()._apply(fn, recurse)
        if self.h.dtype != torch.long:
            self.h = h.to(self.h.device)
        return self

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        if prefix + "h" in state_dict:
            _check_hashes(state_dict[prefix + "h"], self.input_size, self.output_size, prefix + "h")
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, x):
        assert x.shape[-1] == self.input_size
        return ops.CountSketchFn.apply(self.h, self.s, self.output_size, x)


class CompactBilinearPooling(nn.Module):
    def __init__(self, input1_size, input2_size, output_size, h1=None, s1=None, h2=None, s2=None,
                 force_cpu_scatter_add=False):
        super().__init__()
        self.add_module("sketch1", CountSketch(input1_size, output_size, h1, s1))
        self.add_module("sketch2", CountSketch(input2_size, output_size, h2, s2))
        self.output_size = output_size
        self.force_cpu_scatter_add = force_cpu_scatter_add

    def forward(self, x, y=None):
        if y is None:
            y = x
        return ops.CompactBilinearPoolingFn.apply(self.sketch1.h, self.sketch1.s, self.sketch2.h, self.sketch2.s,
                                                  self.output_size, x, y)
