"""CPU: the dispatch decisions and the small-shape arithmetic behind tests/test_gpu_conv2d_arms.py, on the emulation library.

  * test_conv2d_arm_case_reaches_its_arm: every case and variant of tests/conv2d_arm_cases.py with the kernel bodies skipped
    (MVS_EMUL_DRY_LAUNCH=1: argument checks, c2_run_igemm / mvs_conv2d_dgrad_wl / mvs_conv2d_wgrad / wg2_plan and the launch trace are
    host code): only the TRACE is asserted, through mvs_amd.ops.
  * test_conv2d_arm_case_numbers_on_the_emulation: the cases of at most four tiles with the bodies run, by the GPU test's criteria
    (fp64 truth, ATen fp32 yardstick, absolute bounds, statistic slots, canaries behind buffers of exactly the queried size).  The
    larger cases run with MVS_EMUL_FULL=1 (the emulation runs a thread per lane).
  * the rejections: error, empty trace, nothing launched."""
import ctypes as C
import os

import pytest
import torch

import conv2d_arm_cases as K
from emul_util import emul_lib  # noqa: F401

FULL = os.environ.get("MVS_EMUL_FULL", "0") == "1"


@pytest.fixture
def dry_launch(monkeypatch):
    monkeypatch.setenv("MVS_EMUL_DRY_LAUNCH", "1")


@pytest.mark.parametrize("case", K.ALL, ids=K.ids(K.ALL))
def test_conv2d_arm_case_reaches_its_arm(emul_lib, dry_launch, case):
    inp = K.make_inputs(case)
    for v in case.variants:
        with emul_lib.tuning(**v.knobs):
            emul_lib.launch_trace()
            K.run(case, inp, emul_lib, v)
            assert emul_lib.launch_trace() == v.trace, "%s/%s" % (case.id, v.name)


def test_case_table_names_every_arm():
    """each launch label of the conv2d arms appears in at least one case's expected trace, and no case expects a label the library
    does not have"""
    seen = {lab for c in K.ALL for v in c.variants for lab in v.trace}
    assert set(K.ARM_LABELS) <= seen, sorted(set(K.ARM_LABELS) - seen)
    assert seen <= set(K.ARM_LABELS), sorted(seen - set(K.ARM_LABELS))
    assert len({c.id for c in K.ALL}) == len(K.ALL)
    for c in K.ALL:
        names = [v.name for v in c.variants]
        assert len(set(names)) == len(names) and all(a in names and b in names and kind in ("equal", "close") for a, b, kind in c.pairs), c.id


def test_every_label_of_the_source_is_in_the_table():
    """the labels are literals of csrc/conv2d.hip's tables: every "conv2d_igemm / conv2d_dgrad_s2 / conv2d_wgrad" literal the source
    can emit (the label macros expanded by hand in ARM_LABELS) starts with the text the launch check had before the labels were
    split, so a reader that matched the old text still matches"""
    old = ("conv2d_igemm", "conv2d_igemm (pixel pairs)", "conv2d_dgrad_s2_one_pass", "conv2d_dgrad_s2_classes", "conv2d_dgrad_s2", "conv2d_wgrad",
           "conv2d_wgrad_reduce", "conv2d_wgrad_batch", "conv2d_wgrad_batch_reduce", "conv2d_pack_weights_batch")
    for lab in K.ARM_LABELS:
        assert any(lab == o or lab.startswith(o + " ") for o in old), lab


def _small(case):
    return K.tiles(case) <= 4


NUMERIC = [c for c in K.ALL if FULL or _small(c)]


@pytest.mark.parametrize("case", NUMERIC, ids=K.ids(NUMERIC))
def test_conv2d_arm_case_numbers_on_the_emulation(emul_lib, case):
    K.check_numbers(case, emul_lib, torch.device("cpu"), lambda c, i, lib, v: [K.run_owned(c, i, lib, v)])


def test_batched_weight_gradient_work_split(emul_lib):
    """wg2_plan under each wgrad2d_batch value of the table: the workspace it asks for is that of the work split written out in
    tests/conv2d_arm_cases.py (tiles per workgroup = ceil(tiles / share): a floor gives other workgroup counts)"""
    pinned = 0
    for case in K.WGRAD_BATCH:
        for v in case.variants:
            if "ws_floats" in v.opts:
                with emul_lib.tuning(**v.knobs):
                    assert K.batch_ws_query(case, emul_lib)[0] == v.opts["ws_floats"], "%s/%s" % (case.id, v.name)
                pinned += 1
    assert pinned >= 6


def test_numeric_subset_reaches_every_kind_of_arm():
    """what the default run leaves to MVS_EMUL_FULL=1 is size, not kind: each group of the table has cases of <= 4 tiles"""
    for name, grp in K.GROUPS.items():
        if name != "WGRAD_REDUCE":             # (18 and 65 tiles by construction)
            assert any(_small(c) for c in grp), name


# ---- rejections: an error code and message, an empty trace, nothing launched -------------------------------------------------------
def _x(n, c, h, w):
    return torch.zeros(n, c, h, w).contiguous(memory_format=K.CL)


@pytest.mark.parametrize("ks,stride", [(3, 2), (5, 1), (7, 1), (1, 1)])
def test_conv2d_rejects_other_kernel_sizes_and_strides(emul_lib, ks, stride):
    from mvs_amd import ops
    emul_lib.launch_trace()
    ho = (8 - 1) // stride + 1
    with pytest.raises(ValueError, match="unsupported shape"):
        ops.conv2d_forward(_x(1, 8, 8, 8), torch.zeros(8, 8, ks, ks), None, stride)
    with pytest.raises(ValueError, match="unsupported shape"):
        ops.conv2d_dgrad(_x(1, 8, ho, ho), torch.zeros(8, 8, ks, ks), (1, 8, 8, 8), stride)
    with pytest.raises(ValueError, match="unsupported shape"):
        ops.conv2d_wgrad(_x(1, 8, 8, 8), _x(1, 8, ho, ho), (8, 8, ks, ks), stride)
    # the entry points themselves (the wrappers stop at the workspace query)
    buf = torch.zeros(4096)
    p = buf.data_ptr()
    for name, args in (("mvs_conv2d_fwd", (p, p, None, p, p, 1, 8, 8, 8, 8, ks, stride, None)),
                       ("mvs_conv2d_dgrad", (p, p, p, p, 1, 8, 8, 8, 8, ks, stride, None)),
                       ("mvs_conv2d_wgrad", (p, p, p, p, 1, 8, 8, 8, 8, ks, stride, None))):
        assert emul_lib.raw(name, *args) == -2 and b"supports 3x3 stride 1 and 5x5 stride 2" in emul_lib.raw("mvs_last_error")
    assert emul_lib.launch_trace() == []


@pytest.mark.parametrize("cin,cout", [(33, 8), (8, 48), (63, 63), (65, 8), (8, 0)])
def test_conv2d_rejects_33_to_63_channels(emul_lib, cin, cout):
    emul_lib.launch_trace()
    buf = torch.zeros(4096)
    p = buf.data_ptr()
    for name, args in (("mvs_conv2d_fwd", (p, p, None, p, p, 1, 2, 3, cin, cout, 3, 1, None)),
                       ("mvs_conv2d_lrelu_fwd", (p, p, None, p, p, 1, 2, 3, cin, cout, 3, 1, 0.1, None)),
                       ("mvs_conv2d_fwd_stats", (p, p, p, p, p, 4, 1, 1, 2, 3, cin, cout, 3, 1, 0, None)),
                       ("mvs_conv2d_dgrad", (p, p, p, p, 1, 2, 3, cin, cout, 3, 1, None)),
                       ("mvs_conv2d_wgrad", (p, p, p, p, 1, 2, 3, cin, cout, 3, 1, None))):
        assert emul_lib.raw(name, *args) == -2, name
        msg = emul_lib.raw("mvs_last_error")
        assert b"channels must be 1..64" in msg or b"more than 32 channels means exactly 64" in msg, msg
    assert emul_lib.raw("mvs_conv2d_workspace_floats", 2, 1, 2, 3, cin, cout, 3, 1) == -1
    assert emul_lib.launch_trace() == []


def test_conv2d_wgrad_batch_rejections(emul_lib):
    """layers without an instantiation (CG % 4 != 0, CX = 4) and the _xf form over its groups x 2 x CX <= 512 limit"""
    from mvs_amd import ops
    emul_lib.launch_trace()
    for cin, cout in ((8, 6), (4, 8), (8, 20), (32, 36)):
        xs, gys, ws = [_x(1, cin, 2, 3)], [_x(1, cout, 2, 3)], [torch.zeros(cout, cin, 3, 3)]
        assert not ops.conv2d_wgrad_batch_serves(xs, ws, [1])
        with pytest.raises(ValueError, match="not served"):
            ops.conv2d_wgrad_batch(xs, gys, ws, [1])
        shapes = (C.c_int * 8)(1, 2, 3, cin, cout, 3, 1, 0)
        assert emul_lib.raw("mvs_conv2d_wgrad_batch_workspace_floats", 1, shapes) == -1
        buf = torch.zeros(8192)
        ptrs = ops._ptr_array([buf])
        assert emul_lib.raw("mvs_conv2d_wgrad_batch", 1, ptrs, ptrs, ptrs, buf.data_ptr(), shapes, None) == -2
        assert b"without an instantiation" in emul_lib.raw("mvs_last_error")
    # 16 groups x 2 x 32 channels = 1024 floats of (scale, shift) > 512; 8 groups fit
    xs, gys, ws = [_x(16, 32, 1, 1)], [_x(16, 32, 1, 1)], [torch.zeros(32, 32, 3, 3)]
    stats = K._in_stats(torch.Generator().manual_seed(0), 16, 32)
    with pytest.raises(ValueError, match="conv2d_wgrad_batch_xf: layer 0: 32 channels / 16 images in groups of 1"):
        ops.conv2d_wgrad_batch(xs, gys, ws, [1], x_stats=[stats], groups=16)
    assert emul_lib.launch_trace() == []
    ops.conv2d_wgrad_batch(xs, gys, ws, [1], x_stats=[stats[:8].contiguous()], groups=8)
    assert emul_lib.launch_trace() == K.BATCH_XF


@pytest.mark.parametrize("cout", [16, 64])
@pytest.mark.parametrize("ks,cin", K.WGRAD_GAP)
def test_conv2d_wgrad_refuses_what_it_has_no_instantiation_for(emul_lib, ks, cin, cout):
    """The served set of mvs_conv2d_wgrad is narrower than c2_check's: the workspace query says -1, the wrapper raises the workspace
    query's ValueError (before, Conv2dFn / Conv2dLReLUFn of such a layer ran forward and failed in backward with a positive workspace
    size in hand), and the entry point refuses the layer before its first launch -- also with Cout = 64, where a slice loop runs."""
    from mvs_amd import ops
    stride = 2 if ks == 5 else 1
    emul_lib.launch_trace()
    assert emul_lib.raw("mvs_conv2d_workspace_floats", 2, 1, 4, 6, cin, cout, ks, stride) == -1
    assert emul_lib.raw("mvs_conv2d_workspace_floats", 0, 1, 4, 6, cin, cout, ks, stride) > 0      # (the forward pass serves the layer)
    ho, wo = K.out_hw((4, 6), stride)
    with pytest.raises(ValueError, match="conv2d: unsupported shape .*weight gradient"):
        ops.conv2d_wgrad(_x(1, cin, 4, 6), _x(1, cout, ho, wo), (cout, cin, ks, ks), stride)
    buf = torch.full((1 << 16,), float("nan"))
    p = buf.data_ptr()
    assert emul_lib.raw("mvs_conv2d_wgrad", p, p, p, p, 1, 4, 6, cin, cout, ks, stride, None) == -2
    assert b"input channels not served" in emul_lib.raw("mvs_last_error")
    assert emul_lib.launch_trace() == []


@pytest.mark.parametrize("ks,cin", K.WGRAD_SERVED)
def test_conv2d_wgrad_query_accepts_what_it_serves(emul_lib, dry_launch, ks, cin):
    from mvs_amd import ops
    stride = 2 if ks == 5 else 1
    assert emul_lib.raw("mvs_conv2d_workspace_floats", 2, 1, 4, 6, cin, 16, ks, stride) > 0
    emul_lib.launch_trace()
    ho, wo = K.out_hw((4, 6), stride)
    ops.conv2d_wgrad(_x(1, cin, 4, 6), _x(1, 16, ho, wo), (16, cin, ks, ks), stride)
    trace = emul_lib.launch_trace()
    assert len(trace) == (3 if cin == 64 else 2) and trace[-1] == K.NARROW and all(t.startswith("conv2d_wgrad k%d cxp" % ks) for t in trace[:-1])
