"""The ResNet-18 trunk's bf16 data path (option "bf16" = 1: bgemm.h, conv64::kernel<B16, .>, the <true> forms of the BatchNorm
and pooling kernels, pack_all's bf16 packs) on the GPU against the value-pinned float64 replay of tests/trunk_ref.py: every
case under the default options, the schedule options on the cases where the restated table says a bf16 form changes, one
gradient subset and one accumulating run.  The implementation's 17 stored activations (``ops.trunk_saved_activations``:
exact float32 copies of the bf16 storage) and its pool arg-max plane are read after the forward and before the backward;
the replay continues with them layer by layer, so each layer is held to the forward rule given exact inputs and the backward
is the backward of the network the implementation ran.  tests/test_trunk_bf16_cpu.py runs the same cases with the float32
stand-in in the place of the HIP path.  There is no aggregate bound anywhere."""
import pytest
import torch

import trunk_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAG = "gpu"


def trunk_gpu16(inp, frozen, accumulate=False):
    from avvad import _lib as L
    from avvad import nn as avnn
    from avvad import ops
    assert L.get_option("bf16") == 1
    m = avnn.make_resnet18_trunk()
    m.load_state_dict(inp.sd)
    m = m.to(DEV)
    assert [k for k, _ in m.named_parameters()] == R.param_keys()
    for k, p in m.named_parameters():
        p.requires_grad = k not in frozen
        if accumulate and k not in frozen:
            p.grad = R.prefill(k, p.shape).to(DEV)
    f = avnn.trunk_forward(m, inp.x.to(DEV), inp.training)
    acts = {k: v.cpu().contiguous() for k, v in ops.trunk_saved_activations(f).items()}
    argmax = ops.trunk_saved_pool_argmax(f).cpu().contiguous()
    (f * inp.G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: (None if p.grad is None else p.grad.cpu()) for k, p in m.named_parameters()}
    stats = {k: v.cpu() for k, v in m.state_dict().items() if k.rsplit(".", 1)[-1] in ("running_mean", "running_var")}
    return dict(feat=f.detach().cpu(), grads=grads, stats=stats, acts=acts, argmax=argmax)


@pytest.mark.parametrize("case", list(R.CASES))
def test_trunk_bf16_default_options(case, lib_options):
    """the 17 stored layers by the forward rule, the pool positions, features, the 60 parameter gradients and the 40 running
    statistics of every case (what each reaches: ``trunk_ref.forms16``, asserted by the CPU test)"""
    lib_options("bf16", 1)
    R.check_trunk_bf16(trunk_gpu16, case, tag=TAG)


VARIANT_RUNS = sorted(((case, label, options) for label, options, cases in R.VARIANTS16 for case in cases), key=lambda r: r[0])


@pytest.mark.parametrize("case,label,options", VARIANT_RUNS, ids=["%s-%s" % r[:2] for r in VARIANT_RUNS])
def test_trunk_bf16_option_variants(case, label, options, lib_options):
    """every schedule option on a case where it changes a bf16 kernel form (``trunk_ref.forms16``)"""
    lib_options("bf16", 1)
    for k, v in options.items():
        lib_options(k, v)
    R.check_trunk_bf16(trunk_gpu16, case, options_label=label, tag=TAG, options=options)


def test_trunk_bf16_stem_frozen(lib_options):
    """the stem backward skipped: what is not wanted has no gradient, what is wanted is unchanged"""
    lib_options("bf16", 1)
    R.check_trunk_bf16(trunk_gpu16, "T1", frozen=R.frozen_keys("stem_frozen"), options_label="stem_frozen", tag=TAG)


def test_trunk_bf16_gradients_accumulate(lib_options):
    lib_options("bf16", 1)
    R.check_trunk_bf16(lambda inp, frozen: trunk_gpu16(inp, frozen, accumulate=True), "T7", accumulate=True, tag=TAG)


def test_fp32_accessor_is_a_view_and_bf16_a_copy(lib_options):
    """``ops.trunk_saved_activations``: the fp32 path hands out views of the workspace as before; the bf16 path decodes the
    bf16 storage at the same offsets into float32 copies, and the arg-max plane is the same plane in both"""
    from avvad import nn as avnn
    from avvad import ops
    inp = R.inputs("T7")
    m = avnn.make_resnet18_trunk()
    m.load_state_dict(inp.sd)
    m = m.to(DEV)
    f32 = avnn.trunk_forward(m, inp.x.to(DEV), False)
    a32, am32 = ops.trunk_saved_activations(f32), ops.trunk_saved_pool_argmax(f32)
    ws = f32.grad_fn.saved_tensors[1] if type(f32.grad_fn).__name__ == "TrunkFnBackward" else None
    lib_options("bf16", 1)
    f16 = avnn.trunk_forward(m, inp.x.to(DEV), False)
    a16, am16 = ops.trunk_saved_activations(f16), ops.trunk_saved_pool_argmax(f16)
    assert torch.equal(am32, am16)                   # (the stem runs its fp32 kernels in both)
    for k in R.NAMES:
        assert a32[k].dtype == a16[k].dtype == torch.float32 and a32[k].shape == a16[k].shape
        if ws is not None:
            assert a32[k].untyped_storage().data_ptr() == ws.untyped_storage().data_ptr(), k
        assert torch.equal(a16[k].bfloat16().float(), a16[k]), k
    assert torch.equal(a16["pool"], a32["pool"].bfloat16().float())          # the same fp32 value, stored as bf16


def test_zz_log_worst_ratios():
    """(last in the file) worst error / bound per family and the per-run counts go to the parity log"""
    R.log_worst16(TAG)
