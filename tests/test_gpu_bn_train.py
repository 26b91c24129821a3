"""Train-mode BatchNorm kernels of csrc/bn.hip on the MI355X, each on its own against fp64 autograd: the cases of
tests/test_bn_train.py at the same shapes (case code, criteria and input construction: tests/bn_train_cases.py), with real fp64 atomics
and many workgroups in flight.  The measured error ratios of a run go to bn_parity_ratios.jsonl (BT.Record); the copy kept with the
project is profiles/bn_parity_ratios.jsonl."""
import pytest
import torch

import bn_train_cases as BT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("rows", [105, 4096])
@pytest.mark.parametrize("C", BT.CHANNELS)
def test_train_kernels_vs_fp64_autograd(dev, C, rows, relu, with_skip):
    BT.matrix_case(dev, C, rows, relu, with_skip)


@pytest.mark.parametrize("many", [False, True])
@pytest.mark.parametrize("which", ["one", "recommended", "max"])
@pytest.mark.parametrize("C", [4, 8, 64])
def test_slot_row_counts(dev, C, which, many):
    BT.slot_rows_case(dev, C, which, many)


@pytest.mark.parametrize("rows", [BT.ROWS_STATS_CAP, BT.ROWS_ALL_CAPS])
def test_grid_caps(dev, rows):
    BT.grid_cap_case(dev, rows)


@pytest.mark.parametrize("G,Vg,C,ndim", BT.GROUP_CASES)
def test_groups(dev, G, Vg, C, ndim):
    BT.groups_case(dev, G, Vg, C, ndim)


@pytest.mark.parametrize("C,rows,G", [(4, 105, 1), (16, 4096, 1), (32, 105 * 3, 3), (8, 128, 64)])
def test_finalize_is_the_forward_prologue(dev, C, rows, G):
    BT.finalize_case(dev, C, rows, G)


@pytest.mark.parametrize("C", BT.EVAL_CHANNELS)
def test_eval_affine(dev, C):
    BT.eval_affine_case(dev, C)


@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("rows", [105, BT.ROWS_ALL_CAPS])
def test_eval_apply(dev, rows, relu, with_skip):
    """rows 105 and the grid-cap size (n4 just over 2048*256: a ragged second grid-stride pass; device only)"""
    BT.eval_apply_case(dev, rows, relu, with_skip)


@pytest.mark.parametrize("ndim", [4, 5])
def test_bn_relu_fn_backward_twice(dev, ndim):
    BT.backward_twice_case(dev, ndim)


def test_train_entry_points_reject_bad_arguments(dev):
    BT.argument_checks_case(dev)


@pytest.mark.parametrize("ratio", BT.SWEEP_RATIOS)
@pytest.mark.parametrize("C,rows", BT.SWEEP_SHAPES)
def test_conditioning_sweep(dev, C, rows, ratio):
    BT.conditioning_case(dev, C, rows, ratio)
