"""The training FeaturePyramid of CVP-MVSNet as one autograd node on the MI355X: the cases of tests/test_pyramid.py at the same
shapes (case code: tests/pyramid_cases.py), the device activities of one pass under torch.profiler, and CVPMVSNet with the node against
the reference's fixture."""
import pytest
import torch

import pyramid_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("N,H,W,S", PC.IMAGE_SHAPES)
def test_image_pyramid_vs_chained_fp64_interpolate(dev, N, H, W, S):
    PC.images_case(dev, N, H, W, S)


def test_image_pyramid_refuses_a_level_without_pixels(dev):
    PC.images_refuse_case(dev)


@pytest.mark.parametrize("N,H,W", PC.DGRAD_SHAPES)
@pytest.mark.parametrize("cin,cout", PC.DGRAD_CHANNELS)
def test_masked_input_gradient_and_its_records(dev, cin, cout, N, H, W):
    PC.masked_dgrad_case(dev, cin, cout, N, H, W)


@pytest.mark.parametrize("N,H,W", PC.DGRAD_SHAPES)
def test_head_mask_is_leaky_relu_backward(dev, N, H, W):
    PC.head_case(dev, N, H, W)


@pytest.mark.parametrize("N,H,W,S", PC.NODE_SHAPES)
def test_node_vs_per_layer_path_vs_fp64_restatement(dev, N, H, W, S):
    PC.node_case(dev, N, H, W, S)


def test_node_with_the_finest_level_gradient_only(dev):
    PC.node_case(dev, *PC.NODE_SHAPES[0], only_finest=True)


def test_two_backward_passes_give_the_same_bits(dev):
    PC.determinism_case(dev)


def test_launch_trace_of_one_pass(dev):
    PC.launch_trace_case(dev)


def test_every_device_activity_of_a_pass_is_this_librarys_kernel(dev):
    PC.no_foreign_kernel_case(dev)


def test_what_does_not_take_the_node(dev):
    PC.fallback_case(dev)


def test_cvpmvsnet_with_the_node_vs_reference_fixture(dev):
    PC.fixture_case(dev)
