"""The fusion head on the GPU -- MCB fusion (csrc/mcb.hip and the C = 1024 use of csrc/bn_kernels.h), LSTM stack
(csrc/lstm.hip), losses (csrc/misc.hip) -- against the float64 references of tests/head_ref.py, at the smallest shapes that
reach the code paths training runs: several statistics chunks, ragged last chunks, grid-stride loops, long recurrences, the
stride loops of the one-workgroup losses.  The cases, bounds and assertion functions are head_ref's; tests/test_head_cpu.py
runs the same cases with the float32 CPU oracle in the place of the HIP path.  Every case feeds the head kernels directly."""
import pytest
import torch

import head_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAG = "gpu"


def _dev(t):
    return t.to(DEV)


def _leaf(t):
    return t.to(DEV).requires_grad_(True)


# ------------------------------------------------------------------------------------------ MCB fusion
def fusion_gpu(inp, training):
    """``ops.McbFusionFn`` forward + backward; the implementation's own pooled vector comes from ``CompactBilinearPooling``
    (avvad_mcb_fwd launches the mcb_fwd_kernel the fusion launches: the same bits)"""
    from avvad import ops
    from packages.models.compact_bilinear_pooling import CompactBilinearPooling
    h1, s1, h2, s2 = _dev(inp.h1), _dev(inp.s1), _dev(inp.h2), _dev(inp.s2)
    with torch.no_grad():
        y = CompactBilinearPooling(inp.A, inp.V, inp.D, inp.h1, inp.s1, inp.h2, inp.s2).to(DEV)(_dev(inp.a), _dev(inp.v))
    a, v, w, b = _leaf(inp.a), _leaf(inp.v), _leaf(inp.bn_w), _leaf(inp.bn_b)
    rm, rv = _dev(inp.rm0).clone(), _dev(inp.rv0).clone()
    out = ops.McbFusionFn.apply(a, v, h1, s1, h2, s2, w, b, rm, rv, R.EPS, training, R.MOMENTUM)
    (out * _dev(inp.G)).sum().backward()
    return dict(y=y, out=out, da=a.grad, dv=v.grad, dw=w.grad, db=b.grad, rm=rm, rv=rv)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", list(R.FUSION_CASES))
def test_fusion(name, training):
    """out, d audio, d video, d bn weight, d bn bias and both running statistics against the y-pinned float64 reference, the
    pooled vector against the float64 pooling (what each case reaches: ``head_ref.FUSION_CASES``)"""
    R.check_fusion(fusion_gpu, name, training, tag=TAG)


def test_fusion_is_the_same_bits_run_to_run():
    """fixed-order sums everywhere (no float atomics): two runs of the two-chunk case F1 agree bit for bit"""
    inp = R.fusion_inputs("F1")
    p, q = fusion_gpu(inp, True), fusion_gpu(inp, True)
    for k in p:
        assert torch.equal(p[k], q[k]), k


# ------------------------------------------------------------------------------------------ raw pooling and sketch
def pooling_gpu(inp):
    from packages.models.compact_bilinear_pooling import CompactBilinearPooling, CountSketch
    G = _dev(inp.G)
    a, v = _leaf(inp.a), _leaf(inp.v)
    y = CompactBilinearPooling(inp.A, inp.V, inp.D, inp.h1, inp.s1, inp.h2, inp.s2).to(DEV)(a, v)
    (y * G).sum().backward()
    x = _leaf(inp.a)
    sk = CountSketch(inp.A, inp.D, inp.h1, inp.s1).to(DEV)(x)
    (sk * G).sum().backward()
    return dict(y=y, da=a.grad, dv=v.grad, sk=sk, dsk=x.grad)


@pytest.mark.parametrize("name", list(R.POOLING_CASES))
def test_pooling_and_sketch(name):
    """``CompactBilinearPooling`` and ``CountSketch`` stand-alone, forward and input gradients: D = 2048 (the second pass of
    the j0 += 1024 loops) and D = 1000 (no multiple of 256)"""
    R.check_pooling(pooling_gpu, name, tag=TAG)


def test_pooling_refuses_an_output_size_beyond_the_lds_buffers():
    """D = 2049: avvad_mcb_fwd / avvad_count_sketch_fwd return EINVAL before any launch"""
    from avvad import AvvadError
    from packages.models.compact_bilinear_pooling import CompactBilinearPooling, CountSketch
    a, v = torch.zeros(2, 5, device=DEV), torch.zeros(2, 4, device=DEV)
    with pytest.raises(AvvadError):
        CompactBilinearPooling(5, 4, 2049).to(DEV)(a, v)
    with pytest.raises(AvvadError):
        CountSketch(5, 2049).to(DEV)(a)


# ------------------------------------------------------------------------------------------ LSTM
class _Stack:
    """what ``ops.lstm_stack`` reads of an nn.LSTM: the flags and the per-layer parameters"""
    bidirectional, bias, proj_size = False, True, 0

    def __init__(self, inp, frozen=(), misalign=False):
        self.num_layers = inp.layers
        self.params = {}
        for k, t in inp.sd.items():
            if misalign and k.startswith("weight_hh"):
                # a contiguous view one float into a larger buffer: data_ptr % 16 == 4
                buf = torch.zeros(t.numel() + 8, device=DEV)
                view = buf[1:1 + t.numel()].view(t.shape)
                view.copy_(t)
                assert view.is_contiguous() and view.data_ptr() % 16 == 4
                p = torch.nn.Parameter(view, requires_grad=k[:-3] not in frozen)
                assert p.data_ptr() == view.data_ptr()
            else:
                p = torch.nn.Parameter(t.to(DEV), requires_grad=k[:-3] not in frozen)
            self.params[k] = p
            setattr(self, k, p)


def lstm_gpu(inp, frozen=()):
    from avvad import ops
    mod = _Stack(inp, frozen, inp.misalign)
    x = _dev(inp.x).requires_grad_("x" not in frozen)
    y = ops.lstm_stack(x, inp.lens, mod)
    (y * _dev(inp.G)).sum().backward()
    grads = {k: p.grad for k, p in mod.params.items()}
    grads["x"] = x.grad
    return y, grads


def test_lstm_L1_persistent_60_steps():
    """B = 16, H = 256, T = 60: forward lstm_persistent_fwd<4> (58 step barriers, each hand-off copy re-used 29 times);
    backward the fused form (EpiLstmBwd in the product's fix-up)"""
    R.check_lstm(lstm_gpu, "L1", tag=TAG)


def test_lstm_L1s_step_kernel_60_steps(lib_options):
    """L1 with lstm_no_persistent = 1: lstm_step_fwd_mfma<1>, 59 launches; backward fused"""
    lib_options("lstm_no_persistent", 1)
    R.check_lstm(lstm_gpu, "L1s", tag=TAG)


@pytest.mark.parametrize("name", ["L2-T2", "L2-T3"])
def test_lstm_L2_no_barrier_and_one_barrier(name):
    """B = 32, H = 256: lstm_persistent_fwd<4> with T = 2 (no barrier) and T = 3 (one); every sequence of the second group of 16
    has length 1 while the first group runs all T steps; backward fused"""
    R.check_lstm(lstm_gpu, name, tag=TAG)


def test_lstm_L3_two_layers_48_sequences():
    """B = 48, H = 512, T = 16, two layers (layer 2: In = 512).  The forward predicate admits B = 16, 32 and multiples of 64
    to the MFMA kernels: 48 sequences (three groups of 16) take the GEMM + lstm_gates_fwd steps; backward fused (B <= 64),
    its 64-row tile ragged"""
    R.check_lstm(lstm_gpu, "L3", tag=TAG)


def test_lstm_L3p_two_layers_persistent_8():
    """L3 with B = 32, which the MFMA kernels admit: lstm_persistent_fwd<8> on 128 workgroups for both layers (layer 2:
    In = 512), two sequence groups; backward fused"""
    R.check_lstm(lstm_gpu, "L3p", tag=TAG)


def test_lstm_L4_c4_head_shape():
    """B = 64, H = 1024, T = 16, the c4 head: lstm_persistent_fwd<16> on 256 workgroups (the per-step lstm_step_fwd_mfma<1>
    if the device cannot hold them at once); backward fused"""
    R.check_lstm(lstm_gpu, "L4", tag=TAG)


def test_lstm_L5_two_sequence_groups_60_steps():
    """B = 128, H = 64, T = 60: lstm_step_fwd_mfma<4> on a (4, 2) grid, two groups of 64 sequences; backward fused through
    H <= 64 (a 128-row product, two row tiles)"""
    R.check_lstm(lstm_gpu, "L5", tag=TAG)


def test_lstm_L6_small_ragged_two_layers():
    """B = 5, H = 20, T = 33, In = 7, two layers: GEMM + lstm_gates_fwd forward; backward fused, its epilogue on a ragged
    5 x 20 tile"""
    R.check_lstm(lstm_gpu, "L6", tag=TAG)


def test_lstm_L7_no_fused_form():
    """B = 80, H = 72, T = 9: B % 64 != 0 and B, H > 64 -- GEMM + gate kernels in both directions (the unfused backward
    product, lstm_gates_bwd per step)"""
    R.check_lstm(lstm_gpu, "L7", tag=TAG)


@pytest.mark.parametrize("name", ["L8-B16", "L8-B3"])
def test_lstm_L8_one_step(name):
    """T = 1: step 0 alone -- the input GEMM and lstm_gates_fwd, no recurrent kernel of either form (the persistent one needs
    T > 1); backward: one lstm_gates_bwd, no recurrent product"""
    R.check_lstm(lstm_gpu, name, tag=TAG)


def test_lstm_L9_misaligned_weight_hh():
    """weight_hh one float into a larger buffer (data_ptr % 16 == 4): forward falls back from the 16-byte-row kernels to
    GEMM + lstm_gates_fwd, backward from the fused form to the plain product with scalar operand loads"""
    R.check_lstm(lstm_gpu, "L9", tag=TAG)


@pytest.mark.parametrize("subset", list(R.LSTM_SUBSETS))
@pytest.mark.parametrize("name", ["L6", "L1-T5"])
def test_lstm_parameter_subsets(name, subset):
    """gradients for a subset only (x without gradient: dx == nullptr, Audio_Net on spectrograms): what is asked for meets the
    bound, what is frozen keeps grad None.  L6: GEMM forms; L1-T5: persistent forward, fused backward"""
    R.check_lstm(lstm_gpu, name, frozen=R.LSTM_SUBSETS[subset], tag=TAG)


def test_lstm_gradients_accumulate_in_place():
    """Two forward + backward passes on leaf nn.Parameters without zeroing (L1 with T = 5): the second pass finds .grad and
    writes into it through ``_grad_target``; the result is 2 x the reference within the bound, and a function registered in
    ``ops.GRAD_SINKS`` sees each parameter once, in the second pass only."""
    from avvad import ops
    inp = R.lstm_inputs("L1-T5")
    _, ref_g = R.lstm_reference("L1-T5")
    mod = _Stack(inp)
    x = _leaf(inp.x)
    G = _dev(inp.G)
    seen = []
    sink = seen.append
    ops.GRAD_SINKS.append(sink)
    try:
        (ops.lstm_stack(x, inp.lens, mod) * G).sum().backward()
        assert seen == []
        first = {k: p.grad for k, p in mod.params.items()}
        assert all(g is not None for g in first.values())
        (ops.lstm_stack(x, inp.lens, mod) * G).sum().backward()
    finally:
        ops.GRAD_SINKS.remove(sink)
    assert sink not in ops.GRAD_SINKS
    assert len(seen) == len(mod.params) and {id(p) for p in seen} == {id(p) for p in mod.params.values()}
    for k, p in mod.params.items():
        assert p.grad is first[k], k                      # written in place
        R.report_grad("lstm", "L1-T5 accumulated d/d" + k, p.grad, 2.0 * ref_g[k], tag=TAG)
    R.report_grad("lstm", "L1-T5 accumulated d/dx", x.grad, 2.0 * ref_g["x"], tag=TAG)


# ------------------------------------------------------------------------------------------ losses
def masked_bce_gpu(inp):
    from avvad import ops
    r = _leaf(inp.logits)
    loss = ops.masked_bce(r, _dev(inp.targets), inp.lens, R.EPS)
    (loss * R.UPSTREAM).backward()
    return loss, r.grad


@pytest.mark.parametrize("name", list(R.MASKED_BCE_CASES))
def test_masked_bce(name):
    """``ops.masked_bce`` value and d logits (upstream factor 3 through scale_by_device_scalar): c2's 15 360 elements with
    lengths 1 .. 60, Y = 3, one element beyond a trip of the 1024-thread stride loop, and saturated logits"""
    R.check_masked_bce(masked_bce_gpu, name, tag=TAG)


def bce_2classes_gpu(inp):
    from packages.models.utils import binary_cross_entropy_2classes
    r1, r2 = _leaf(inp.r1), _leaf(inp.r2)
    loss = binary_cross_entropy_2classes(r1, r2, _dev(inp.x), R.EPS)
    (loss * R.UPSTREAM).backward()
    return loss, r1.grad, r2.grad


def test_bce_2classes():
    """rows = 1367, Y = 3: 4101 elements, five trips of the stride loop"""
    R.check_bce_2classes(bce_2classes_gpu, tag=TAG)


def test_worst_ratios_go_to_the_log():
    R.log_worst(TAG)
