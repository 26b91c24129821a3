"""CPU: the dispatch decisions behind tests/test_gpu_conv_arms.py.  Every case of tests/conv_arm_cases.py is called on the emulation
library with the kernel bodies skipped (MVS_EMUL_DRY_LAUNCH=1: argument checks, run_igemm / run_cin1 / run_wgrad and the launch
trace are host code) and only the TRACE is asserted: a GPU case that stops reaching its arm because a threshold moved fails here
first.  The kernels' arithmetic at the small shapes is test_emul_kernels.py's business, on the GPU test_gpu_conv_arms.py's."""
import pytest
import torch

import conv_arm_cases as K
from emul_util import emul_lib  # noqa: F401


@pytest.fixture
def dry_launch(monkeypatch):
    monkeypatch.setenv("MVS_EMUL_DRY_LAUNCH", "1")


def test_launch_trace_reports_and_clears(emul_lib):
    """mvs_launch_trace: labels since the previous call in launch order, then forgotten; a small buffer gets whole labels only and
    the count still says how many launches there were."""
    import ctypes as C
    from mvs_amd import ops
    emul_lib.launch_trace()
    assert emul_lib.launch_trace() == []
    x, w = torch.randn(1, 8, 2, 3, 5), torch.randn(16, 8, 3, 3, 3)
    ops.conv3d_forward(x, w, 1, False)
    assert emul_lib.launch_trace() == ["conv_pack_weights", "conv_igemm s1_small"]
    assert emul_lib.launch_trace() == []
    ops.conv3d_forward(x, w, 1, False)
    buf = C.create_string_buffer(20)
    assert emul_lib.raw("mvs_launch_trace", buf, 20) == 2 and buf.value == b"conv_pack_weights"
    assert emul_lib.raw("mvs_launch_trace", buf, 20) == 0 and buf.value == b""
    ops.conv3d_forward(x, w, 1, False)
    assert emul_lib.raw("mvs_launch_trace", None, 0) == 2 and emul_lib.launch_trace() == []


@pytest.mark.parametrize("case", K.ALL, ids=K.ids(K.ALL))
def test_conv_arm_case_reaches_its_arm(emul_lib, dry_launch, case):
    inp = K.make_inputs(case)
    for v in ([case.base] if case.base is not None else []) + list(case.variants):
        with emul_lib.tuning(**v.knobs):
            emul_lib.launch_trace()
            K.run(case, inp, emul_lib)
            assert emul_lib.launch_trace() == v.trace, "%s/%s" % (case.id, v.name)


def test_case_table_names_every_arm():
    """each launch label of the convolution arms appears in at least one case's expected trace"""
    seen = {lab for c in K.ALL for v in list(c.variants) + ([c.base] if c.base else []) for lab in v.trace}
    for lab in ("conv_pers nw=8", "conv_pers nw=4", "conv_wgrad_pers", "conv_igemm s1", "conv_igemm s2", "conv_igemm s1_small",
                "conv_igemm s2_small", "conv_igemm tr2_pw", "conv_cout1 h4", "conv_cout1 cin=8", "conv_cout1 cin=16",
                "conv_cin1 vpt=1", "conv_cin1 vpt=4", "conv_wgrad nbw=1", "conv_wgrad nbw=2", "conv_wgrad (small tiles) nbw=1",
                "conv_wgrad (small tiles) nbw=2", "conv_wgrad_reduce wide", "conv_wgrad_reduce narrow", "conv_pack_weights",
                "conv_wgrad_cg1", "conv_c8_fwd_bc", "conv_c8_wgrad", "conv_c8_wgrad_gs"):
        assert lab in seen, lab


@pytest.mark.parametrize("dims", [(5, 8, 10), (6, 7, 10), (6, 8, 9)], ids=["odd_depth", "odd_height", "odd_width"])
def test_conv3d_stride2_input_gradient_rejects_odd_dims(emul_lib, dims):
    """mvs_conv3d_dgrad at stride 2 serves even input dims only (the transposed geometry writes 2 x the output gradient's grid);
    the host names the limit and launches nothing."""
    from mvs_amd import ops
    gy = torch.zeros(2, 32, *[(s - 1) // 2 + 1 for s in dims])
    emul_lib.launch_trace()
    with pytest.raises(ValueError, match=r"conv3d_dgrad stride 2: D,H,W must be even, got %d x %d x %d" % dims):
        ops.conv3d_dgrad(gy, torch.zeros(32, 16, 3, 3, 3), (2, 16) + dims, 2, False)
    assert emul_lib.launch_trace() == []
