"""CPU: the opt-in arithmetic of the frozen trunk's wide convolutions (csrc/conv2d_wide_bf16_kernels.h: ``arith="bf16"``) on the
emulation build, which emulates the 16x16x32 bf16 MFMA.

bf16 is held to the criterion the fp32 arms meet (conftest's: fp64 = truth, fp32 F.conv2d = yardstick) against the convolution of
the bf16-ROUNDED operands: with rounded operands every product is exact, so only the fp32 accumulation differs from the yardstick
and no free tolerance is needed.  Then: the forced arms, operands that are bf16 values already (exact), locality of a NaN, the Cin = 3 layer, a whole small trunk, the plan cache and the
host validation of the new entry points on the product library."""
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_as_accurate_as_fp32_reference
from emul_util import emul_lib  # noqa: F401
from test_vgg_features import (LAYER_CASES, TRUNK_LAYERS, expected_conv_labels, layer_inputs, layer_reference, plan_args, small_trunk)

MODES = ("bf16",)
CASES = LAYER_CASES[1:4]
VARIANTS = [(True, True, False), (False, True, True), (True, False, True), (False, False, False)]    # bias, relu, channels-last parameter


def _id(c):
    return "%dx%dx%d_%dto%d%s" % (c[:5] + ("_pool" if c[5] else "",))


BF_SPLIT_MIN = 2048      # csrc/tuning.h: c2w_bf_split_min, the bf16 arms' own split-K threshold


def mode_labels(mode, m, cin, cout, **knobs):
    """the fp32 rule's labels under the bf16 arms' split-K threshold, with the mode's name in the arm labels"""
    knobs.setdefault("split_min", BF_SPLIT_MIN)
    return [l.replace("conv2d_wide ", "conv2d_wide %s " % mode) if l.split()[1][0] in "ts" else l
            for l in expected_conv_labels(m, cin, cout, **knobs)]


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)       # round to nearest even


def references(mode, x, wt, b, relu, pool):
    """-> (fp32 yardstick, fp64 truth) of a mode: for bf16 the convolution of the rounded operands (bias unrounded)"""
    if mode == "bf16":
        x, wt = bf16_round(x), bf16_round(wt)
    return layer_reference(x, wt, b, relu, pool, torch.float32), layer_reference(x, wt, b, relu, pool, torch.float64)


def run(lib, ops, mode, x, wt, b, relu, pool, wcl=False, **knobs):
    w_in = wt.contiguous(memory_format=torch.channels_last) if wcl else wt
    lib.launch_trace()
    with lib.tuning(**knobs):
        y = ops.conv2d_wide_forward(x.permute(0, 2, 3, 1).contiguous(), w_in, b, relu=relu, pool=pool, arith=mode)
    return y, lib.launch_trace()


@pytest.mark.parametrize("bias,relu,wcl", VARIANTS)
@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("mode", MODES)
def test_layer_vs_conv2d(emul_lib, mode, case, bias, relu, wcl):
    from mvs_amd import ops
    n, h, w, cin, cout, pool = case
    x, wt, b = layer_inputs(case)
    b = b if bias else None
    y, trace = run(emul_lib, ops, mode, x, wt, b, relu, pool, wcl)
    assert trace == ["conv2d_wide %s pack" % mode] + mode_labels(mode, n * h * w, cin, cout) + (["pool2x2"] if pool else [])
    r32, r64 = references(mode, x, wt, b, relu, pool)
    assert tuple(y.shape) == tuple(r64.shape) and y.is_contiguous()
    assert_as_accurate_as_fp32_reference(y, r32, r64, what="conv2d_wide %s %r" % (mode, case))


@pytest.mark.parametrize("case,knobs,labels", [
    (LAYER_CASES[1], dict(c2w_splitk=3), ["conv2d_wide %s splitk=3", "conv2d_wide reduce"]),
    (LAYER_CASES[2], dict(c2w_splitk=8), ["conv2d_wide %s splitk=8", "conv2d_wide reduce", "pool2x2"]),    # 27 steps in ranges of 4: one is empty
    (LAYER_CASES[3], dict(c2w_tile=2, c2w_splitk=1), ["conv2d_wide %s t128x64"]),
])
@pytest.mark.parametrize("mode", MODES)
def test_layer_arms_by_knob(emul_lib, mode, case, knobs, labels):
    from mvs_amd import ops
    x, wt, b = layer_inputs(case)
    y, trace = run(emul_lib, ops, mode, x, wt, b, True, case[5], **knobs)
    assert trace == ["conv2d_wide %s pack" % mode] + [l % mode if "%s" in l else l for l in labels]
    r32, r64 = references(mode, x, wt, b, True, case[5])
    assert_as_accurate_as_fp32_reference(y, r32, r64, what="conv2d_wide %s %r %r" % (mode, case, knobs))
    if knobs.get("c2w_tile") == 2:
        y64, t64 = run(emul_lib, ops, mode, x, wt, b, True, case[5], c2w_tile=1, c2w_splitk=1)
        assert t64[1] == "conv2d_wide %s t64x64" % mode
        assert torch.equal(y, y64)


@pytest.mark.parametrize("case", [LAYER_CASES[1], LAYER_CASES[2]], ids=_id)
def test_operands_that_are_bf16_values(emul_lib, case):
    """small integers times powers of two are bf16 values: the rounding changes nothing, every product and every partial sum is
    exact in fp32, so without a bias the result equals the fp64 convolution to the bit, whatever the order of the accumulation"""
    from mvs_amd import ops
    n, h, w, cin, cout, pool = case
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-7, 8, (n, cin, h, w), generator=g).float() * 2.0 ** torch.randint(-3, 4, (n, cin, h, w), generator=g).float()
    wt = torch.randint(-5, 6, (cout, cin, 3, 3), generator=g).float() * 2.0 ** torch.randint(-6, 0, (cout, cin, 3, 3), generator=g).float()
    assert torch.equal(bf16_round(x), x) and torch.equal(bf16_round(wt), wt)
    y, _ = run(emul_lib, ops, "bf16", x, wt, None, False, pool)
    r64 = layer_reference(x, wt, None, False, pool, torch.float64)
    assert float(y.abs().max()) > 1.0 and torch.equal(y.double(), r64)


@pytest.mark.parametrize("mode", MODES)
def test_a_nan_stays_in_its_neighbourhood(emul_lib, mode):
    """One NaN activation in the last row of image 0 (2x14x14, a tile spans both images): every output outside its 3x3
    neighbourhood, all of image 1 included, has the bits of the run without it -- a border test taken on the tile instead of on
    the row would let it into image 1."""
    from mvs_amd import ops
    case = LAYER_CASES[1]
    x, wt, b = layer_inputs(case)
    y0, _ = run(emul_lib, ops, mode, x, wt, b, False, False)      # (no ReLU: fmaxf would turn the NaN into 0)
    xn = x.clone()
    xn[0, 5, 13, 6] = float("nan")
    y1, _ = run(emul_lib, ops, mode, xn, wt, b, False, False)
    near = torch.zeros(2, 14, 14, dtype=torch.bool)
    near[0, 12:14, 5:8] = True
    assert bool(torch.isnan(y1[near]).all())
    assert torch.equal(y1[~near], y0[~near]) and bool(torch.isfinite(y0).all())


@pytest.mark.parametrize("mode", MODES)
def test_cin3_layer_stays_fp32(emul_lib, mode):
    from mvs_amd import ops
    case = LAYER_CASES[0]
    x, wt, b = layer_inputs(case)
    y, trace = run(emul_lib, ops, mode, x, wt, b, True, False)
    y32, trace32 = run(emul_lib, ops, "f32", x, wt, b, True, False)
    assert trace == ["conv2d_wide pack", "conv2d_wide cin3"] == trace32
    assert torch.equal(y, y32)


def test_arith_names(emul_lib):
    from mvs_amd import ops
    assert [ops.wide_arith(a) for a in ("f32", "bf16", 0, 2)] == [0, 2, 0, 2]
    x, wt, b = layer_inputs(LAYER_CASES[1])
    for bad in ("fp16", "bf16x3", 1, 3, -1, None, True):
        with pytest.raises(ValueError, match="arith must be one of"):
            ops.conv2d_wide_forward(x.permute(0, 2, 3, 1).contiguous(), wt, b, arith=bad)
    y_default = ops.conv2d_wide_forward(x.permute(0, 2, 3, 1).contiguous(), wt, b)
    emul_lib.launch_trace()
    y_f32 = ops.conv2d_wide_forward(x.permute(0, 2, 3, 1).contiguous(), wt, b, arith="f32")
    assert emul_lib.launch_trace() == ["conv2d_wide pack", "conv2d_wide t64x64"] and torch.equal(y_default, y_f32)


# ---- whole small trunk ---------------------------------------------------------------------------------------------------
def test_trunk(emul_lib):
    """The stand-in chain of tests/test_vgg_features.py: arith="f32" through the new entry is bitwise the old entry; bf16 has the
    fp32 trace with the mode's labels, and its relative L1 against the UNROUNDED fp64 network is within 2x that of a torch
    restatement of the mode (every convolution but the first, Cin = 3, with its input and weights rounded to bf16, convolved in
    fp32): both carry the same quantisation noise, and 2x is the slack the project's criterion grants between two fp32
    evaluations (the rule of tests/test_gpu_vgg_features_arith.py::test_whole_trunk_bf16)."""
    import copy
    from mvs_amd import _lib, ops
    from mvs_amd.ops import _p, _stream
    net = small_trunk()
    x = torch.randn(2, 3, 32, 48, generator=torch.Generator().manual_seed(9))
    x_cl = x.permute(0, 2, 3, 1).contiguous()
    ops._TRUNK_PLANS.clear()
    plan = ops.trunk_plan(plan_args(net), x_cl.shape, x_cl)
    emul_lib.launch_trace()
    old = ops.conv_trunk_forward(plan, x_cl)
    trace_old = emul_lib.launch_trace()
    new = torch.empty_like(old)
    emul_lib.call("mvs_conv_trunk_fwd_arith", plan.n_layers, plan.table, plan.packed_ptrs, plan.bias_ptrs, _p(x_cl), _p(plan.buf_a),
                  _p(plan.buf_b), _p(plan.ws), _p(new), 2, 32, 48, 0, _stream(x_cl))
    assert emul_lib.launch_trace() == trace_old and torch.equal(new, old)

    plan3 = ops.trunk_plan(plan_args(net), x_cl.shape, x_cl, arith="bf16")
    pack_trace = emul_lib.launch_trace()
    assert pack_trace == ["conv2d_wide pack"] + ["conv2d_wide bf16 pack"] * 15
    y3 = ops.conv_trunk_forward(plan3, x_cl)
    trace3 = emul_lib.launch_trace()
    want, m, cin = [], 2 * 32 * 48, 3
    for v in TRUNK_LAYERS:
        if v == "M":
            want.append("pool2x2")
            m //= 4
        else:
            want += mode_labels("bf16", m, cin, v)
            cin = v
    assert trace3 == want and "conv2d_wide bf16 splitk=2" in want and "conv2d_wide bf16 t64x64" in want and want[0] == "conv2d_wide cin3"
    with torch.no_grad():
        r64 = copy.deepcopy(net).double().features(x.double()).permute(0, 2, 3, 1)
        t = x
        for m in net.features:
            if isinstance(m, torch.nn.Conv2d) and m.in_channels != 3:
                t = F.conv2d(bf16_round(t), bf16_round(m.weight), m.bias, padding=1)
            else:
                t = m(t)
        restated = t.permute(0, 2, 3, 1)
    assert tuple(y3.shape) == (2, 2, 3, 96) and float(r64.abs().max()) > 0.05
    norm = float(r64.abs().sum())
    e_ours, e_restated = float((y3.double() - r64).abs().sum()) / norm, float((restated.double() - r64).abs().sum()) / norm
    print("trunk bf16: relative L1 against the fp64 network: ours %.3e, torch restatement %.3e" % (e_ours, e_restated))
    assert e_restated > 1e-4 and e_ours <= 2.0 * e_restated
    # a bad arith: rejected before the first launch
    with pytest.raises(ValueError, match="arith must be 0"):
        emul_lib.call("mvs_conv_trunk_fwd_arith", plan.n_layers, plan.table, plan.packed_ptrs, plan.bias_ptrs, _p(x_cl), _p(plan.buf_a),
                      _p(plan.buf_b), _p(plan.ws), _p(new), 2, 32, 48, 1, _stream(x_cl))
    assert emul_lib.launch_trace() == []


def test_plan_cache_is_per_arith(emul_lib):
    from mvs_amd import ops
    layers = (32, "M", 32)
    net = small_trunk(layers, seed=5)
    x = torch.randn(1, 3, 6, 4, generator=torch.Generator().manual_seed(6))
    x_cl = x.permute(0, 2, 3, 1).contiguous()
    ops._TRUNK_PLANS.clear()

    def run_(arith):
        emul_lib.launch_trace()
        plan = ops.trunk_plan(plan_args(net), x_cl.shape, x_cl, arith=arith)
        y = ops.conv_trunk_forward(plan, x_cl)
        return y, [t for t in emul_lib.launch_trace() if t.endswith("pack")]

    y0, p0 = run_("f32")
    y1, p1 = run_("bf16")
    y2, p2 = run_("bf16")
    y3, p3 = run_("f32")
    assert emul_lib.get_tuning("c2w_bf_split_min") == BF_SPLIT_MIN
    assert p0 == ["conv2d_wide pack"] * 2 and p1 == ["conv2d_wide pack", "conv2d_wide bf16 pack"] and p2 == [] and p3 == []
    assert torch.equal(y1, y2) and torch.equal(y0, y3) and float((y1 - y0).abs().max()) > 0.0


def test_segdff_feature_arith_arguments():
    import seg_oracle as S
    from mvs_amd.jdacs.losses.unsup_seg_loss import UnSupSegLoss
    from mvs_amd.jdacs.models.seg_dff import SegDFF, vgg19_trunk
    from mvs_amd.jdacs_ms.losses.unsup_seg_loss import UnSupSegLoss as MsLoss
    from mvs_amd.jdacs_ms.models.seg_dff import SegDFF as MsSegDFF
    vgg = vgg19_trunk()
    assert SegDFF(4, net=vgg).feature_arith == "f32" and SegDFF.HIP_FEATURES_DEFAULT is True
    m = MsSegDFF(4, net=vgg, feature_arith="bf16")
    assert m.feature_arith == "bf16" and m.hip_features is True
    assert MsLoss(4, net=vgg, hip_features=True, feature_arith="bf16").seg_model.feature_arith == "bf16"
    assert UnSupSegLoss(4, net=vgg).seg_model.feature_arith == "f32"
    with pytest.raises(ValueError, match="hip_features=False"):
        SegDFF(4, net=vgg, hip_features=False, feature_arith="bf16")
    with pytest.raises(ValueError, match="not a trunk the HIP kernels serve"):
        SegDFF(4, net=S.StandInNet(), feature_arith="bf16")
    with pytest.raises(ValueError, match="arith must be one of"):
        UnSupSegLoss(4, net=vgg, feature_arith="bf16x3")


# ---- host validation, on the product library ----------------------------------------------------------------------------
def test_error_convention_of_the_arith_entry_points():
    from mvs_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.MvsLib()
    for arith in (0, 2):
        with pytest.raises(ValueError, match="null pointer"):
            lib.call("mvs_conv2d_wide_pack_weights_arith", None, None, 64, 64, 0, arith, None)
        with pytest.raises(ValueError, match="null pointer"):
            lib.call("mvs_conv2d_wide_fwd_arith", None, None, None, None, None, 1, 8, 8, 64, 64, 1, 0, arith, None)
        with pytest.raises(ValueError, match="null pointer"):
            lib.call("mvs_conv_trunk_fwd_arith", 1, None, None, None, None, None, None, None, None, 1, 8, 8, arith, None)
        with pytest.raises(ValueError, match="steps of 32, got 48 -> 64"):
            lib.call("mvs_conv2d_wide_fwd_arith", None, None, None, None, None, 1, 8, 8, 48, 64, 1, 0, arith, None)
        with pytest.raises(ValueError, match="steps of 32, got 64 -> 640"):
            lib.call("mvs_conv2d_wide_pack_weights_arith", None, None, 64, 640, 0, arith, None)
        with pytest.raises(ValueError, match="cannot be pooled"):
            lib.call("mvs_conv2d_wide_fwd_arith", None, None, None, None, None, 1, 1, 8, 64, 64, 1, 1, arith, None)
    for bad in (1, 3, -1):
        for name, args in [("mvs_conv2d_wide_pack_weights_arith", (None, None, 64, 64, 0, bad, None)),
                           ("mvs_conv2d_wide_fwd_arith", (None, None, None, None, None, 1, 8, 8, 64, 64, 1, 0, bad, None)),
                           ("mvs_conv_trunk_fwd_arith", (1, None, None, None, None, None, None, None, None, 1, 8, 8, bad, None))]:
            with pytest.raises(ValueError, match=r"failed \(-2\): .*arith must be 0 \(f32\) or 2 \(bf16\), got %d" % bad):
                lib.call(name, *args)            # -2: MVS_ERR_UNSUPPORTED
        assert lib.raw("mvs_conv2d_wide_packed_bytes_arith", 64, 64, bad) == -1
        assert lib.raw("mvs_conv2d_wide_workspace_floats_arith", 1, 8, 8, 64, 64, bad) == -1
    assert lib.launch_trace() == []
    assert lib.raw("mvs_conv2d_wide_packed_bytes_arith", 48, 64, 2) == -1
    # fp32 image: 18 steps x 2 halves x 8 column tiles x 256 floats; bf16 image: 18 steps x 8 column tiles x 64 lanes x 16 bytes
    assert lib.raw("mvs_conv2d_wide_packed_bytes_arith", 64, 96, 0) == 4 * lib.raw("mvs_conv2d_wide_packed_floats", 64, 96) == 4 * 18 * 2 * 8 * 256
    assert lib.raw("mvs_conv2d_wide_packed_bytes_arith", 64, 96, 2) == 18 * 8 * 64 * 16
    # Cin = 3 keeps the fp32 image (and the fp32 arm) in every mode
    assert [lib.raw("mvs_conv2d_wide_packed_bytes_arith", 3, 64, a) for a in (0, 2)] == [4 * 2 * 4 * 256] * 2
    assert lib.raw("mvs_conv2d_wide_workspace_floats_arith", 7, 14, 14, 512, 512, 0) == lib.raw("mvs_conv2d_wide_workspace_floats", 7, 14, 14, 512, 512)
    assert lib.raw("mvs_conv2d_wide_workspace_floats_arith", 7, 224, 224, 64, 64, 2) == 7 * 224 * 224 * 64
    # the bf16 arms split K under c2w_bf_split_min = 2048 workgroups: 176 at 14x14 -> eight ranges, 688 at 28x28 -> four
    assert lib.raw("mvs_conv2d_wide_workspace_floats_arith", 7, 14, 14, 512, 512, 2) == 1372 * 512 * 9
    assert lib.raw("mvs_conv2d_wide_workspace_floats_arith", 7, 28, 28, 512, 512, 2) == 5488 * 512 * 5
    assert lib.raw("mvs_conv2d_wide_workspace_floats_arith", 7, 28, 28, 512, 512, 0) == 5488 * 512
    assert lib.raw("mvs_conv2d_wide_workspace_floats_arith", 7, 56, 56, 256, 256, 2) == 7 * 56 * 56 * 256      # t128x64: never split
