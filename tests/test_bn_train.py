"""Train-mode BatchNorm kernels of csrc/bn.hip on the CPU emulation of the kernel sources (tests/cpu_emul), each against fp64 autograd
with the stock fp32 ops (A) and the scheme's own formula in plain torch (B) as the yardsticks.  The same cases run on the device in
tests/test_gpu_bn_train.py; the case code, the criteria and the construction of the inputs are tests/bn_train_cases.py."""
import pytest
import torch

import bn_train_cases as BT
from emul_util import emul_lib  # noqa: F401

CPU = torch.device("cpu")


def test_input_construction_holds_for_every_seeded_case():
    """no pre-activation within 1e-3 of zero, a channel that is closed everywhere, a constant channel: asserted inside
    BT.inputs for every (C, rows, G, ratio) any case of either suite uses -- without a kernel, so a seed that breaks the
    construction shows here first"""
    for C in BT.CHANNELS:
        for rows in BT.DIMS:
            BT.inputs(C, rows)
    for C, (few, many) in BT.SLOT_ROWS.items():
        BT.inputs(C, few), BT.inputs(C, many)
    for rows in (BT.ROWS_ALL_CAPS, BT.ROWS_STATS_CAP):
        BT.inputs(8, rows)
    for G, Vg, C, _ in BT.GROUP_CASES:
        BT.inputs(C, G * Vg, G)
    BT.inputs(16, 480, 2)
    for C, rows in BT.SWEEP_SHAPES:
        for ratio in BT.SWEEP_RATIOS:
            inp = BT.inputs(C, rows, 1, ratio)
            x = inp.x.double()
            got = x.mean(0).abs() / x.std(0, unbiased=False).clamp_min(1e-30)
            normal = [c for c in range(C) if c != BT.CONST_CH]
            assert bool(((got[normal] - ratio).abs() <= 1e-4 * max(1, ratio)).all()), "the sample mean/std is not the ratio asked for"


@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("rows", [105, 4096])
@pytest.mark.parametrize("C", BT.CHANNELS)
def test_train_kernels_vs_fp64_autograd(emul_lib, C, rows, relu, with_skip):
    BT.matrix_case(CPU, C, rows, relu, with_skip)


@pytest.mark.parametrize("many", [False, True])
@pytest.mark.parametrize("which", ["one", "recommended", "max"])
@pytest.mark.parametrize("C", [4, 8, 64])
def test_slot_row_counts(emul_lib, C, which, many):
    """nslots 1 / mvs_bn_slots / 256 with fewer workgroups than slot rows (unused rows stay zero) and with more (rows wrap);
    C = 4 x 256 rows sits on the boundary of bn_slot_totals' eight-load prologue, C = 8 and C = 64 x 256 rows run its tail loop"""
    BT.slot_rows_case(CPU, C, which, many)


@pytest.mark.parametrize("rows", [BT.ROWS_STATS_CAP, BT.ROWS_ALL_CAPS])
def test_grid_caps(emul_lib, rows):
    """n4 just over 512*256 (only bn_stats_slots takes a second grid-stride pass) and just over 2048*256 (every kernel takes a ragged one)"""
    BT.grid_cap_case(CPU, rows)


@pytest.mark.parametrize("G,Vg,C,ndim", BT.GROUP_CASES)
def test_groups(emul_lib, G, Vg, C, ndim):
    BT.groups_case(CPU, G, Vg, C, ndim)


@pytest.mark.parametrize("C,rows,G", [(4, 105, 1), (16, 4096, 1), (32, 105 * 3, 3), (8, 128, 64)])
def test_finalize_is_the_forward_prologue(emul_lib, C, rows, G):
    BT.finalize_case(CPU, C, rows, G)


@pytest.mark.parametrize("C", BT.EVAL_CHANNELS)
def test_eval_affine(emul_lib, C):
    BT.eval_affine_case(CPU, C)


@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("relu", [1, 0])
def test_eval_apply(emul_lib, relu, with_skip):
    """rows 105 here; the grid-cap size of this kernel runs on the device only (tests/test_gpu_bn_train.py): 2049 emulated workgroups
    of 256 host threads per launch take too long for this suite"""
    BT.eval_apply_case(CPU, 105, relu, with_skip)


@pytest.mark.parametrize("ndim", [4, 5])
def test_bn_relu_fn_backward_twice(emul_lib, ndim):
    BT.backward_twice_case(CPU, ndim)


def test_train_entry_points_reject_bad_arguments(emul_lib):
    BT.argument_checks_case(CPU)


@pytest.mark.parametrize("ratio", BT.SWEEP_RATIOS)
@pytest.mark.parametrize("C,rows", BT.SWEEP_SHAPES)
def test_conditioning_sweep(emul_lib, C, rows, ratio):
    BT.conditioning_case(CPU, C, rows, ratio)
