"""The stage glue of a CVPMVSNet forward (csrc/cvp_stage_kernels.h) on the MI355X: the cases of tests/test_cvp_stage.py (case code:
tests/cvp_stage_cases.py), the model against the g7 and g13 fixtures with the stage on, and the device activities of one forward under
torch.profiler with the stage off and on."""
import pytest
import torch

import cvp_stage_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("H,W", SC.UP_SHAPES)
def test_level_transition_vs_fp64_restatement_oracle_and_todays_path(dev, H, W):
    SC.up_case(dev, H, W)


def test_level_transition_of_the_g7_fixture(dev):
    SC.up_fixture_case(dev)


def test_level_transition_refuses_bad_arguments(dev):
    SC.up_refuse_case(dev)


@pytest.mark.parametrize("B,S,L,img_h,level_hs", SC.CAMERA_CASES)
def test_cameras_vs_exact_rational_arithmetic(dev, B, S, L, img_h, level_hs):
    assert len(level_hs) == L
    SC.cameras_case(dev, SC.camera_inputs(B, S, img_h, img_h * 5 // 4), img_h, level_hs, "synthetic B%d S%d L%d h%d" % (B, S, L, img_h))


@pytest.mark.parametrize("name", ("g7", "g13"))
def test_cameras_of_the_fixtures_vs_exact_rational_arithmetic(dev, name):
    cams = SC.fixture_cameras(name)
    SC.cameras_case(dev, cams[:6], cams[6], cams[7], name)


def test_cameras_refuse_bad_arguments(dev):
    SC.cameras_refuse_case(dev)


def test_launch_trace_of_a_forward_stage_on_and_off(dev):
    SC.launch_trace_case(dev)


def test_g7_fixture_stage_on_and_off(dev):
    SC.g7_case(dev)


def test_g13_fixture_with_gradients_stage_on(dev):
    SC.g13_case(dev)


def test_device_activities_of_a_forward_stage_off_and_on(dev):
    SC.profiler_case(dev)
