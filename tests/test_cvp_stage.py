"""The stage glue of a CVPMVSNet forward (csrc/cvp_stage_kernels.h) on the CPU emulation of the kernel sources (tests/cpu_emul): the
cases of tests/cvp_stage_cases.py -- the level transition against the fp64 restatement, the oracle and today's path; the cameras
against exact rational arithmetic; the model's launch trace and fallbacks.  tests/test_gpu_cvp_stage.py runs the same cases on the
device.  The emulation runs a thread per lane and pays over a minute for a regulariser pass: the model's launch-trace case takes a
16x16 image here (the GPU suite: 32x48) with a channel mean in the regulariser's place, which the glue under test neither runs nor
reads; the real regulariser and the g7 fixture case run with MVS_EMUL_FULL=1, like the other long emulation cases of this suite, and
the g13 fixture case with its backward pass runs on the device only."""
import os

import pytest
import torch

import cvp_stage_cases as SC
from emul_util import emul_lib  # noqa: F401

DEV = torch.device("cpu")
FULL = os.environ.get("MVS_EMUL_FULL", "0") == "1"


@pytest.fixture(autouse=True)
def _lib(emul_lib):
    return emul_lib


@pytest.mark.parametrize("H,W", SC.UP_SHAPES)
def test_level_transition_vs_fp64_restatement_oracle_and_todays_path(H, W):
    SC.up_case(DEV, H, W)


def test_level_transition_of_the_g7_fixture():
    SC.up_fixture_case(DEV)


def test_level_transition_refuses_bad_arguments():
    SC.up_refuse_case(DEV)


@pytest.mark.parametrize("B,S,L,img_h,level_hs", SC.CAMERA_CASES)
def test_cameras_vs_exact_rational_arithmetic(B, S, L, img_h, level_hs):
    assert len(level_hs) == L
    SC.cameras_case(DEV, SC.camera_inputs(B, S, img_h, img_h * 5 // 4), img_h, level_hs, "synthetic B%d S%d L%d h%d" % (B, S, L, img_h))


@pytest.mark.parametrize("name", ("g7", "g13"))
def test_cameras_of_the_fixtures_vs_exact_rational_arithmetic(name):
    cams = SC.fixture_cameras(name)
    SC.cameras_case(DEV, cams[:6], cams[6], cams[7], name)


def test_cameras_refuse_bad_arguments():
    SC.cameras_refuse_case(DEV)


def test_launch_trace_of_a_forward_stage_on_and_off():
    SC.launch_trace_case(DEV, 16, 16, stub_regulariser=not FULL)


@pytest.mark.skipif(not FULL, reason="minutes of emulation; set MVS_EMUL_FULL=1 (the GPU version is test_gpu_cvp_stage.py::test_g7_fixture_stage_on_and_off)")
def test_g7_fixture_stage_on_and_off():
    SC.g7_case(DEV)
