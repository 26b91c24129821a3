"""RefineNet on the MI355X: the cases of tests/test_refine.py at the same shapes (case code: tests/refine_cases.py), the device
kernels of a refine train step under torch.profiler, and MVSNet(refine=True) against the reference's fixture."""
import pytest
import torch

import refine_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W", RC.ASSEMBLE_SHAPES)
def test_assembly_is_interpolate_plus_cat_within_one_ulp(dev, H, W, B):
    RC.assemble_case(dev, B, H, W)


def test_assembly_refuses_a_depth_map_of_another_size(dev):
    RC.assemble_refuses_other_depth_sizes_case(dev)


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("rows", RC.TAIL_ROWS)
def test_one_channel_tail_vs_fp64_autograd(dev, rows, frozen):
    RC.tail_case(dev, rows, frozen)


@pytest.mark.parametrize("h,w", [(5, 7), (33, 41)])
def test_eval_tail_is_the_folded_convolution(dev, h, w):
    RC.eval_tail_case(dev, h, w)


@pytest.mark.parametrize("B,h,w", RC.MODULE_SHAPES)
@pytest.mark.parametrize("mode", RC.MODES)
def test_refinenet_hip_pass_vs_stock_vs_fp64_oracle(dev, mode, B, h, w):
    RC.modes_case(dev, mode, B, h, w)


def test_launch_trace_shows_the_refine_kernels(dev):
    RC.launch_trace_case(dev)


def test_refine_train_step_runs_no_library_kernel(dev):
    RC.no_library_kernel_case(dev)


def test_a_mix_of_batchnorm_modes_takes_the_per_block_path(dev):
    RC.fallback_case(dev)


def test_mvsnet_with_refine_vs_reference_fixture(dev):
    RC.fixture_case(dev)
