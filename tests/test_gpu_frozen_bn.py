"""Frozen-statistics BatchNorm with a gradient on the MI355X: the cases of tests/test_frozen_bn.py at the same shapes (case code:
tests/frozen_bn_cases.py), the model-level cases in both ways of freezing, and one frozen step at a benchmark size."""
import copy

import pytest
import torch

import frozen_bn_cases as FB
from conftest import assert_grads_as_accurate_as_fp32_reference
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("form", ["none", "computed", "prefilled"])
@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("rows", [105, 4096])
@pytest.mark.parametrize("C", FB.KERNEL_CHANNELS)
def test_frozen_backward_kernels_vs_fp64_autograd(dev, C, rows, relu, with_skip, form):
    FB.kernel_case(dev, C, rows, relu, with_skip, form)


@pytest.mark.parametrize("mode", ["idiom", "eval"])
@pytest.mark.parametrize("which", list(FB.BLOCKS_3D))
def test_frozen_3d_block_trains_through_and_leaves_statistics_alone(dev, which, mode):
    FB.block3d_case(dev, which, mode)


@pytest.mark.parametrize("which", list(FB.BLOCKS_3D))
def test_eval_3d_block_without_gradient_is_the_folded_convolution(dev, which):
    FB.block3d_no_grad_case(dev, which)


@pytest.mark.parametrize("c,groups", [(4, 1), (8, 3), (32, 2), (64, 1)])
def test_frozen_bn_relu_2d(dev, c, groups):
    FB.bn_relu_2d_case(dev, c, groups)


@pytest.mark.parametrize("cin,cout,k,stride", [(8, 16, 3, 1), (16, 32, 5, 2)])
@pytest.mark.parametrize("mode", ["idiom", "eval"])
def test_frozen_2d_block(dev, mode, cin, cout, k, stride):
    """on the device the block's BatchNorm runs through ops.BnReLUFn: under the idiom it took batch statistics and moved the running
    ones before the frozen path existed"""
    FB.block2d_case(dev, mode, cin, cout, k, stride)


@pytest.mark.parametrize("which", ["mvs", "cvp"])
def test_frozen_regulariser_one_node_vs_per_layer(dev, which):
    FB.costreg_case(dev, which)


def test_regulariser_with_one_training_batchnorm_takes_the_per_layer_graph(dev):
    FB.costreg_mixed_case(dev, "mvs")


def test_frozen_mvsnet_vs_reference_fixture(dev):
    ours = FB.mvsnet_case(dev, "idiom")
    frozen_affine = FB.mvsnet_case(dev, "idiom", affine_grads=False)
    for k, v in frozen_affine.items():
        assert FB.rel_l1(v, ours[k]) < 1e-4, k


def test_mvsnet_in_eval_mode_with_autograd_on(dev):
    """model.eval() + backward(): the reference cannot (its eval branch works in place); the drop-in computes the same step as
    under the idiom"""
    FB.mvsnet_case(dev, "eval")


def test_frozen_cvpmvsnet_vs_reference_fixture(dev):
    FB.cvp_case(dev)


def test_frozen_step_at_config_1_size(dev):
    """One frozen MVSNet step at BASELINE config 1's size (N=3, 160x128, D=48) -- the fp64 oracle on the CPU that serves as the
    truth takes minutes at config 2's 640x512, D=192 --: finite, statistics untouched, one-node and per-layer frozen gradients both
    as accurate as the fp32 oracle's."""
    from mvs_amd import ops
    from mvs_amd.jdacs.models.mvsnet import MVSNet
    from conftest import calibrate_batchnorm
    torch.manual_seed(0)
    net = MVSNet(refine=False)
    with torch.no_grad():
        net.cost_regularization.prob.weight.mul_(50.0)
    imgs, proj, dv = R.synthetic_mvsnet_inputs(1, 3, 128, 160, 48, seed=1)
    oracle = R.OracleMVSNet(refine=False)
    oracle.load_state_dict(net.state_dict())
    calibrate_batchnorm(oracle, imgs, proj, dv)
    net.load_state_dict(oracle.state_dict())
    refs = {}
    for dtype in (torch.float32, torch.float64):
        o = FB.freeze_batchnorm(copy.deepcopy(oracle).to(dtype))
        o(imgs.to(dtype), proj.to(dtype), dv.to(dtype))["depth"].mean().backward()
        refs[dtype] = {k: p.grad for k, p in o.named_parameters() if not k.endswith("prob.bias")}
    net = FB.freeze_batchnorm(net.to(dev))
    before = FB.buffers_of(net)
    for fused in (True, False):
        net.zero_grad(set_to_none=True)
        old = ops.FUSED_REGULARISER
        ops.FUSED_REGULARISER = fused
        try:
            out = net(imgs.to(dev), proj.to(dev), dv.to(dev))
            out["depth"].mean().backward()
        finally:
            ops.FUSED_REGULARISER = old
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out["depth"]).all())
        FB.assert_buffers_untouched(before, net, "config-1 frozen step")
        ours = {k: p.grad.cpu() for k, p in net.named_parameters() if k in refs[torch.float32]}
        assert all(bool(torch.isfinite(v).all()) for v in ours.values())
        assert_grads_as_accurate_as_fp32_reference(ours, refs[torch.float32], refs[torch.float64],
                                                   what="frozen config-1 step, %s" % ("one node" if fused else "per layer"))
