"""RefineNet on HIP, on the CPU emulation of the kernel sources (tests/cpu_emul): the cases of tests/refine_cases.py -- input
assembly, the one-channel tail (batch and frozen statistics), the folded eval tail, and RefineNet(hip_pass=True) against the stock
path and the fp64 oracle in every mode.  tests/test_gpu_refine.py runs the same cases on the device."""
import pytest
import torch

import refine_cases as RC
from emul_util import emul_lib  # noqa: F401

DEV = torch.device("cpu")


@pytest.fixture(autouse=True)
def _lib(emul_lib):
    return emul_lib


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W", RC.ASSEMBLE_SHAPES)
def test_assembly_is_interpolate_plus_cat_bit_for_bit(H, W, B):
    RC.assemble_case(DEV, B, H, W)


def test_assembly_refuses_a_depth_map_of_another_size():
    RC.assemble_refuses_other_depth_sizes_case(DEV)


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("rows", RC.TAIL_ROWS)
def test_one_channel_tail_vs_fp64_autograd(rows, frozen):
    RC.tail_case(DEV, rows, frozen)


@pytest.mark.parametrize("h,w", [(5, 7), (33, 41)])
def test_eval_tail_is_the_folded_convolution(h, w):
    RC.eval_tail_case(DEV, h, w)


@pytest.mark.parametrize("B,h,w", RC.MODULE_SHAPES)
@pytest.mark.parametrize("mode", RC.MODES)
def test_refinenet_hip_pass_vs_stock_vs_fp64_oracle(mode, B, h, w):
    RC.modes_case(DEV, mode, B, h, w)


def test_launch_trace_shows_the_refine_kernels():
    RC.launch_trace_case(DEV)


def test_a_mix_of_batchnorm_modes_takes_the_per_block_path():
    RC.fallback_case(DEV)
