"""The ResNet-18 trunk on the GPU (csrc/trunk.hip, igemm.h, conv64.h, bn_kernels.h) -- forward + backward through
``avvad.nn.trunk_forward`` -- against the decision-pinned float64 reference of tests/trunk_ref.py: every case under the default
options (N >= 128 with ragged class tiles feeding fused statistics, H != W, odd stem grids, a 1x1 last stage, wide grids),
the schedule options that change a kernel form on the cases that tell them apart, subsets of the gradients, and accumulation.
The cases, the decision rule, the bounds and the assertion function are trunk_ref's; tests/test_trunk_cpu.py runs the same
cases with the float32 CPU evaluation in the place of the HIP path.  Every run is ONE case under ONE option set; the HIP path's
decisions (the 17 saved sign patterns, the pool's arg-max plane) are read after the forward and before the backward, which
frees the saved workspace.  There is no aggregate bound anywhere."""
import pytest
import torch

import trunk_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAG = "gpu"


def trunk_gpu(inp, frozen, accumulate=False):
    from avvad import nn as avnn
    from avvad import ops
    m = avnn.make_resnet18_trunk()
    m.load_state_dict(inp.sd)
    m = m.to(DEV)
    assert [k for k, _ in m.named_parameters()] == R.param_keys()
    for k, p in m.named_parameters():
        p.requires_grad = k not in frozen
        if accumulate and k not in frozen:
            p.grad = R.prefill(k, p.shape).to(DEV)
    f = avnn.trunk_forward(m, inp.x.to(DEV), inp.training)
    masks = {k: (v > 0).cpu() for k, v in ops.trunk_saved_activations(f).items()}
    argmax = ops.trunk_saved_pool_argmax(f).cpu().contiguous()
    (f * inp.G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: (None if p.grad is None else p.grad.cpu()) for k, p in m.named_parameters()}
    stats = {k: v.cpu() for k, v in m.state_dict().items() if k.rsplit(".", 1)[-1] in ("running_mean", "running_var")}
    return dict(feat=f.detach().cpu(), grads=grads, stats=stats, masks=masks, argmax=argmax)


@pytest.mark.parametrize("case", list(R.CASES))
def test_trunk_default_options(case):
    """features, the 60 parameter gradients and the 40 running statistics of every case (what each reaches:
    ``trunk_ref.CASES``, asserted by the CPU test)"""
    R.check_trunk(trunk_gpu, case, tag=TAG)


VARIANT_RUNS = sorted(((case, label, options) for label, options, cases, _ in R.VARIANTS for case in cases), key=lambda r: r[0])


@pytest.mark.parametrize("case,label,options", VARIANT_RUNS, ids=["%s-%s" % r[:2] for r in VARIANT_RUNS])
def test_trunk_option_variants(case, label, options, lib_options):
    """every schedule option that changes a kernel form of the case (``trunk_ref.forms``; bwd_max_cus: the backward takes
    other forms than the forward did)"""
    for k, v in options.items():
        lib_options(k, v)
    R.check_trunk(trunk_gpu, case, options_label=label, tag=TAG)


@pytest.mark.parametrize("subset", list(R.SUBSETS))
@pytest.mark.parametrize("case", ["T7", "T1"])
def test_trunk_gradient_subsets(case, subset):
    """what is not wanted has no gradient (``grad is None``), what is wanted is unchanged: the stem backward skipped,
    weight gradients without BatchNorm's and the reverse, one block alone"""
    R.check_trunk(trunk_gpu, case, frozen=R.frozen_keys(subset), options_label=subset, tag=TAG)


@pytest.mark.parametrize("case", ["T7", "T1"])
def test_trunk_gradients_accumulate(case):
    """every gradient is added to what .grad already holds (the kernels' ``+=`` forms)"""
    R.check_trunk(lambda inp, frozen: trunk_gpu(inp, frozen, accumulate=True), case, accumulate=True, tag=TAG)


def test_zz_log_worst_ratios():
    """(last in the file) the worst error / bound per family and the decisions that differed go to the parity log"""
    R.log_worst(TAG)
