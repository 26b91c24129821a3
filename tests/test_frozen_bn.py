"""Frozen-statistics BatchNorm with a gradient, on the CPU emulation of the kernel sources (tests/cpu_emul): the kernels of
csrc/bn.hip against fp64 autograd, the 3-D / 2-D blocks and both regularisers against the stock modules, and the two drop-in models
against fixtures written from the live reference under the freeze idiom (tests/golden/make_golden_frozen_bn.py).  The same cases run
on the device in tests/test_gpu_frozen_bn.py; the case code is tests/frozen_bn_cases.py."""
import os

import pytest
import torch

import frozen_bn_cases as FB
from emul_util import emul_lib  # noqa: F401

CPU = torch.device("cpu")


@pytest.mark.parametrize("form", ["none", "computed", "prefilled"])
@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("rows", [105, 4096])
@pytest.mark.parametrize("C", FB.KERNEL_CHANNELS)
def test_frozen_backward_kernels_vs_fp64_autograd(emul_lib, C, rows, relu, with_skip, form):
    """draw bit-identical to scale*dyh in fp32; dgamma / dbeta within 2e-4 relative + 2e-2 absolute of the fp64 sums; the three
    forms: no affine gradient (one launch, no reduction), sums computed by the pass, sums pre-filled by an input-gradient epilogue"""
    FB.kernel_case(CPU, C, rows, relu, with_skip, form)


def test_frozen_entry_points_reject_bad_arguments(emul_lib):
    from mvs_amd import ops
    x = torch.randn(1, 12, 2, 2, 2).contiguous(memory_format=FB.CL3)
    stats = torch.zeros(4, 12)
    with pytest.raises(Exception, match="4/8/16/32/64"):
        ops.bn_relu_bwd_frozen(x, x, stats, want_affine=False)
    x8 = torch.randn(1, 8, 2, 2, 2).contiguous(memory_format=FB.CL3)
    dg = torch.zeros(8)
    assert emul_lib.raw("mvs_bn_relu_bwd_frozen", ops._p(x8), ops._p(x8), ops._p(torch.zeros(4, 8)), None, 0, 0, 1, 8, 8, ops._p(x8.clone()),
                        ops._p(dg), None, None) != 0          # an affine gradient without slot rows
    assert emul_lib.raw("mvs_bn_frozen_stats", None, None, None, None, 1e-5, 8, None, None) != 0


@pytest.mark.parametrize("mode", ["idiom", "eval"])
@pytest.mark.parametrize("which", list(FB.BLOCKS_3D))
def test_frozen_3d_block_trains_through_and_leaves_statistics_alone(emul_lib, which, mode):
    """fails without the frozen path: under the idiom the block took batch statistics and overwrote running_mean / running_var /
    num_batches_tracked; in .eval() backward() raised NotImplementedError"""
    FB.block3d_case(CPU, which, mode)


@pytest.mark.parametrize("which", list(FB.BLOCKS_3D))
def test_eval_3d_block_without_gradient_is_the_folded_convolution(emul_lib, which):
    FB.block3d_no_grad_case(CPU, which)


@pytest.mark.parametrize("c,groups", [(4, 1), (8, 3), (32, 2), (64, 1)])
def test_frozen_bn_relu_2d(emul_lib, c, groups):
    """ops.BnReLUFn(training=False).backward raised NotImplementedError before the frozen path existed"""
    FB.bn_relu_2d_case(CPU, c, groups)


@pytest.mark.parametrize("mode", ["idiom", "eval"])
def test_frozen_2d_block(emul_lib, mode):
    FB.block2d_case(CPU, mode)


@pytest.mark.parametrize("which", ["mvs", "cvp"])
def test_frozen_regulariser_one_node_vs_per_layer(emul_lib, which):
    FB.costreg_case(CPU, which)


def test_regulariser_with_one_training_batchnorm_takes_the_per_layer_graph(emul_lib):
    FB.costreg_mixed_case(CPU, "mvs")


def test_frozen_mvsnet_vs_reference_fixture(emul_lib):
    """MVSNet under the freeze idiom vs g18_frozen_bn_mvs (the live reference, same idiom): depth rel_l1 < 1e-3, every parameter
    gradient and the image gradient as accurate as the reference's fp32 ones (fp64 oracle as truth), statistics bit-identical; then
    gamma / beta with requires_grad=False: the same weight gradients, None for the affine ones"""
    ours = FB.mvsnet_case(CPU, "idiom")
    frozen_affine = FB.mvsnet_case(CPU, "idiom", affine_grads=False)
    for k, v in frozen_affine.items():
        assert FB.rel_l1(v, ours[k]) < 1e-5, k


@pytest.mark.skipif(os.environ.get("MVS_EMUL_FULL") != "1", reason="minutes of emulation (two pyramid levels through the 64-channel "
                    "regulariser); set MVS_EMUL_FULL=1 -- the same case runs on the GPU in tests/test_gpu_frozen_bn.py")
def test_frozen_cvpmvsnet_vs_reference_fixture(emul_lib):
    FB.cvp_case(CPU)
