"""The training FeaturePyramid of CVP-MVSNet as one autograd node, on the CPU emulation of the kernel sources (tests/cpu_emul): the
cases of tests/pyramid_cases.py -- the image pyramid, the masked input gradient with its records, the head, the node against the
per-layer path and the fp64 restatement, determinism, the launch trace, the fallbacks.  tests/test_gpu_pyramid.py runs the same cases
on the device.  The emulation runs a thread per lane: the node cases take PC.EMUL_NODE_SHAPE by default and the shapes of the GPU
suite (40-220 s each here) with MVS_EMUL_FULL=1, like the other long emulation cases of this suite."""
import os

import pytest
import torch

import pyramid_cases as PC
from emul_util import emul_lib  # noqa: F401

DEV = torch.device("cpu")
FULL = os.environ.get("MVS_EMUL_FULL", "0") == "1"
NODE_SHAPES = (PC.EMUL_NODE_SHAPE,) + (PC.NODE_SHAPES if FULL else ())
FIRST = PC.NODE_SHAPES[0] if FULL else PC.EMUL_NODE_SHAPE


@pytest.fixture(autouse=True)
def _lib(emul_lib):
    return emul_lib


@pytest.mark.parametrize("N,H,W,S", PC.IMAGE_SHAPES)
def test_image_pyramid_vs_chained_fp64_interpolate(N, H, W, S):
    PC.images_case(DEV, N, H, W, S)


def test_image_pyramid_refuses_a_level_without_pixels():
    PC.images_refuse_case(DEV)


@pytest.mark.parametrize("N,H,W", PC.DGRAD_SHAPES)
@pytest.mark.parametrize("cin,cout", PC.DGRAD_CHANNELS)
def test_masked_input_gradient_and_its_records(cin, cout, N, H, W):
    PC.masked_dgrad_case(DEV, cin, cout, N, H, W)


@pytest.mark.parametrize("N,H,W", PC.DGRAD_SHAPES)
def test_head_mask_is_leaky_relu_backward(N, H, W):
    PC.head_case(DEV, N, H, W)


@pytest.mark.parametrize("N,H,W,S", NODE_SHAPES)
def test_node_vs_per_layer_path_vs_fp64_restatement(N, H, W, S):
    PC.node_case(DEV, N, H, W, S)


def test_node_with_the_finest_level_gradient_only():
    PC.node_case(DEV, *FIRST, only_finest=True)


def test_two_backward_passes_give_the_same_bits():
    PC.determinism_case(DEV, FIRST)


def test_launch_trace_of_one_pass():
    PC.launch_trace_case(DEV)


def test_what_does_not_take_the_node():
    PC.fallback_case(DEV)
