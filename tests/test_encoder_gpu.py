"""The WaveNet encoder on the GPU (csrc/wavenet.hip, wn_block.h, wn_tail.h) -- forward + backward of
``packages.models.wavenet_autoencoder`` -- against the flip-aware float64 reference of tests/encoder_ref.py: every case under
the default options, every form of the block forward, of the input gradient, of the dz + weight-gradient pass and of the tail
backward on the cases that tell them apart, subsets of the gradients, and accumulation.  The cases, bounds and the assertion
function are encoder_ref's; tests/test_encoder_cpu.py runs the same cases with the float32 CPU oracle in the place of the HIP
path.  Unlike the form-agreement tests of test_gpu_parity.py, every run here is held to an absolute reference, so a fault in
a body that all forms share does not cancel."""
import pytest
import torch

import encoder_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAG = "gpu"

FORM_CASES = ("E1r", "E2", "E3")
BLOCK1 = {"dil_w": "en_dilation_layer_stack.1.weight", "dense_w": "en_dense_layer_stack.1.weight",
          "dil_b": "en_dilation_layer_stack.1.bias", "dense_b": "en_dense_layer_stack.1.bias",
          "bott_w": "bottleneck_layer.weight"}
# wave without gradient (dwave == NULL: how training runs), the five frozen sets of test_wavenet_partially_frozen_blocks,
# everything frozen in block 1 (its backward takes the UNFUSED path)
SUBSETS = {
    "wave_without_grad": ("wave",),
    "dil_w": ("dil_w",), "dense_w": ("dense_w",), "dil_w+dense_w": ("dil_w", "dense_w"), "dil_b+dense_b": ("dil_b", "dense_b"),
    "bott_w": ("bott_w",),
    "whole_block_1": ("dil_w", "dil_b", "dense_w", "dense_b"),
}


def encoder_gpu(inp, frozen, passes=1):
    from packages.models.wavenet_autoencoder import wavenet_autoencoder
    m = wavenet_autoencoder(**inp.cfg)
    m.load_state_dict(inp.params)
    m = m.to(DEV)
    names = [k for k, _ in m.named_parameters()]
    assert sorted(names) == sorted(inp.params)
    for k, p in m.named_parameters():
        p.requires_grad = k not in frozen
    wave = inp.wave.to(DEV).requires_grad_("wave" not in frozen)
    G = inp.G.to(DEV)
    for _ in range(passes):
        out = m(wave)
        ((out * G).sum() * R.UPSTREAM).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads["wave"] = wave.grad
    return dict(out=out.detach(), grads=grads)


@pytest.mark.parametrize("name", list(R.CASES))
def test_encoder_default_options(name):
    """out, d wave and every parameter gradient of every case (what each reaches: ``encoder_ref.CASES``)"""
    R.check_encoder(encoder_gpu, name, tag=TAG)


@pytest.mark.parametrize("flat", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", ["E1r", "E2", "E3", "E9"])
def test_encoder_forward_forms(name, flat, lib_options):
    """the five forms of the block forward: flat, resident, dwordx4, high occupancy, LDS-DMA"""
    lib_options("wn_flat", flat)
    R.check_encoder(encoder_gpu, name, tag=TAG, label="wn_flat=%d" % flat)


def test_encoder_forward_on_a_capped_grid(lib_options):
    """E3 on 8 workgroups: 32 waves walk 140 tiles"""
    lib_options("wn_grid", 8)
    R.check_encoder(encoder_gpu, "E3", tag=TAG, label="wn_grid=8")


@pytest.mark.parametrize("option", [("wn_bwd_t", 1), ("wn_bwd_t", 2), ("wn_bwd_t", 3), ("wn_no_fused_wgrad", 1)],
                         ids=lambda o: "%s=%d" % o)
@pytest.mark.parametrize("name", FORM_CASES)
def test_encoder_dz_and_weight_gradient_forms(name, option, lib_options):
    """transposed, high occupancy, resident weights, and z / dz / weight gradients as three kernels"""
    lib_options(*option)
    R.check_encoder(encoder_gpu, name, tag=TAG, label="%s=%d" % option)


@pytest.mark.parametrize("dx", [1, 2, 3])
@pytest.mark.parametrize("name", FORM_CASES)
def test_encoder_input_gradient_forms(name, dx, lib_options):
    """resident weights, high occupancy, and the flat kernel (which runs with the flat forward)"""
    lib_options("wn_dx", dx)
    if dx == 3:
        lib_options("wn_flat", 1)
    R.check_encoder(encoder_gpu, name, tag=TAG, label="wn_dx=%d" % dx)


@pytest.mark.parametrize("option", [None, ("wn_no_tail_pair", 1), ("wn_no_fused_tail", 1)],
                         ids=lambda o: "default" if o is None else "%s=%d" % o)
@pytest.mark.parametrize("name", ["E2", "T1-256", "T2", "T6"])
def test_encoder_tail_backward_forms(name, option, lib_options):
    """Bn = 256: two waves per tile, one wave per tile, and dz_t written out for the engine.  E2 has overlapping bins with
    P <= Lv; T1-256 and T2 have P > Lv, where a sample lies in more bins than the three-register window of those forms
    holds: whatever the options say, they must take a path that walks the full range.  T6 has more time tiles than one
    round of the fused forms takes: a second round with dead pairs, a second stride step, 256 slabs to reduce"""
    if option is not None:
        lib_options(*option)
    R.check_encoder(encoder_gpu, name, tag=TAG, label="tail " + ("default" if option is None else "%s=%d" % option))


@pytest.mark.parametrize("subset", list(SUBSETS))
@pytest.mark.parametrize("name", ["E2", "E6"])
def test_encoder_gradient_subsets(name, subset):
    """what is not wanted has no gradient (``grad is None``), what is wanted is unchanged"""
    frozen = tuple(k if k == "wave" else BLOCK1[k] for k in SUBSETS[subset])
    R.check_encoder(encoder_gpu, name, frozen=frozen, tag=TAG)


def test_encoder_gradients_accumulate():
    """two forward + backward passes without zeroing: every gradient is twice the reference, within the bound"""
    R.check_encoder(lambda inp, frozen: encoder_gpu(inp, frozen, passes=2), "E1r", tag=TAG, label="two passes", passes=2)


def test_zz_log_worst_ratios():
    """(last in the file) the worst error / bound of this run and the number of runs that needed a flip go to the parity log"""
    R.log_worst(TAG)
