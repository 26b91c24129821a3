"""GPU (MI355X): the opt-in arithmetic of the frozen trunk's wide convolutions (csrc/conv2d_wide_bf16_kernels.h, ``arith="bf16"``)
on the device.

Per layer: conftest's criterion (what the fp32 arms are held to) against the convolution of the bf16-rounded operands -- truth =
fp64 F.conv2d of the rounded operands on the device, yardstick = ATen's fp32 convolution of the same (every product exact: only
the fp32 accumulation differs).  Whole VGG19 trunk: against a torch restatement that rounds every convolution's input and weights
to bf16 (see test_whole_trunk_bf16).  Then the equality of the two tiles and of two calls, SegDFF's routing, and no host
synchronisation.

Per-case error ratios are appended to the file MVS_VGG_REPORT names."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import assert_as_accurate_as_fp32_reference
from test_gpu_vgg_features import _case_id, _ratios, _report, dev, vgg  # noqa: F401
from test_vgg_features import LAYER_CASES, expected_conv_labels, layer_inputs, layer_reference

pytestmark = pytest.mark.gpu

MODES = ("bf16",)
# the last two: the bf16 arms' own split-K threshold (c2w_bf_split_min = 2048 t64x64 workgroups; a t64x64 launch has fewer than
# 2 x c2w_big_min = 1024, so what ends the doubling is the eight-range cap or the nine steps every range keeps)
CASES = [(c, "per-layer case") for c in LAYER_CASES[1:4]] + [
    ((1, 14, 14, 512, 512, False), "deepest layer, one image: the most K ranges"),
    ((1, 56, 56, 128, 256, False), "block 3"),
    ((1, 112, 112, 64, 64, True), "pool at full width"),
    ((7, 28, 28, 256, 512, False), "688 t64x64 workgroups: four K ranges where the fp32 arm is unsplit"),
    ((1, 28, 28, 64, 512, False), "18 k-steps: two K ranges, every range keeps nine steps"),
]


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def mode_labels(mode, lib, m, cin, cout):
    return [l.replace("conv2d_wide ", "conv2d_wide %s " % mode) if l.split()[1][0] in "ts" else l
            for l in expected_conv_labels(m, cin, cout, big_min=lib.get_tuning("c2w_big_min"), split_min=lib.get_tuning("c2w_bf_split_min"))]


@pytest.mark.parametrize("idx", range(len(CASES)))
@pytest.mark.parametrize("mode", MODES)
def test_arm_vs_aten(dev, mode, idx):
    from mvs_amd import _lib, ops
    lib = _lib.get()
    case, what = CASES[idx]
    n, h, w, cin, cout, pool = case
    x, wt, b = [t.to(dev) for t in layer_inputs(case)]
    xr, wr = (bf16_round(x), bf16_round(wt)) if mode == "bf16" else (x, wt)
    with torch.no_grad():
        r64 = layer_reference(xr, wr, b, True, pool, torch.float64)
        r32 = layer_reference(xr, wr, b, True, pool, torch.float32)
    x_cl = x.permute(0, 2, 3, 1).contiguous()
    lib.launch_trace()
    y = ops.conv2d_wide_forward(x_cl, wt, b, relu=True, pool=pool, arith=mode)
    trace = lib.launch_trace()
    y2 = ops.conv2d_wide_forward(x_cl, wt.contiguous(memory_format=torch.channels_last), b, relu=True, pool=pool, arith=mode)
    r = _ratios(y, r32, r64)
    print("%s %s (%s): %s  max %.3e vs ATen %.3e, mean %.3e vs %.3e" % (mode, _case_id(case), what, trace[1], r["max_ours"], r["max_aten"],
                                                                       r["mean_ours"], r["mean_aten"]))
    _report(dict(case=_case_id(case), what=what, arith=mode, arm=trace[1:], **r))
    assert trace == ["conv2d_wide %s pack" % mode] + mode_labels(mode, lib, n * h * w, cin, cout) + (["pool2x2"] if pool else [])
    assert torch.equal(y, y2)                  # two calls (the second from a channels-last parameter): the same bits
    assert_as_accurate_as_fp32_reference(y, r32, r64, what="%s %s" % (mode, _case_id(case)))


def _trunk(net, x_cl, arith):
    from mvs_amd import ops
    from mvs_amd.jdacs.models.seg_dff import trunk_layers
    plan = ops.trunk_plan([(m.weight, m.bias, relu, pool) for m, relu, pool in trunk_layers(net)], x_cl.shape, x_cl, arith=arith)
    return ops.conv_trunk_forward(plan, x_cl)


@pytest.fixture(scope="module")
def trunk_refs(dev, vgg):
    """one 224x224 image: (x, the network in fp64 = truth, the network in fp32 = yardstick), both [1,14,14,512]"""
    x1 = torch.rand(7, 3, 224, 224, generator=torch.Generator().manual_seed(3))[:1].contiguous().to(dev)
    with torch.no_grad():
        r64 = copy.deepcopy(vgg).double().features(x1.double()).permute(0, 2, 3, 1).contiguous()
        r32 = vgg.features(x1).permute(0, 2, 3, 1).contiguous()
    return x1, r64, r32


def test_whole_trunk_bf16(dev, vgg, trunk_refs):
    """A rounded-operand truth does not exist end to end (an activation near a rounding boundary may round the other way in an
    fp64 run), so the yardstick is a torch restatement of the mode: every convolution's input and weights rounded to bf16, the
    convolution in fp32 -- except the first (Cin = 3), which stays fp32 in every mode.  Its relative L1 against the UNROUNDED
    fp64 network is the mode's quantisation noise; ours must be within 2x that (both carry the same noise, boundary flips are
    symmetric, and 2x is the slack the project's criterion grants between two fp32 evaluations)."""
    from mvs_amd import _lib
    lib = _lib.get()
    x1, r64, _ = trunk_refs
    with torch.no_grad():
        t = x1
        for m in vgg.features:
            if isinstance(m, nn.Conv2d) and m.in_channels != 3:
                t = F.conv2d(bf16_round(t), bf16_round(m.weight), m.bias, padding=1)
            else:
                t = m(t)
        restated = t.permute(0, 2, 3, 1).contiguous()
    lib.launch_trace()
    y = _trunk(vgg, x1.permute(0, 2, 3, 1).contiguous(), "bf16")
    tr = [t for t in lib.launch_trace() if "pack" not in t]
    assert tr[0] == "conv2d_wide cin3" and sum(t.startswith("conv2d_wide bf16 ") for t in tr) == 15
    norm = float(r64.abs().sum())
    e_ours, e_restated = float((y.double() - r64).abs().sum()) / norm, float((restated.double() - r64).abs().sum()) / norm
    print("trunk bf16 N=1: relative L1 against the fp64 network: ours %.3e, torch restatement %.3e" % (e_ours, e_restated))
    _report(dict(case="vgg19 trunk 1x224x224", what="whole trunk", arith="bf16", rel_l1_ours=e_ours, rel_l1_restated=e_restated))
    assert e_restated > 1e-4          # the yardstick is the mode's noise, not zero
    assert e_ours <= 2.0 * e_restated


@pytest.mark.parametrize("mode", MODES)
def test_tiles_and_calls_give_the_same_bits(dev, mode):
    from mvs_amd import _lib, ops
    lib = _lib.get()
    case = (7, 56, 56, 256, 256, False)
    x, wt, b = [t.to(dev) for t in layer_inputs(case)]
    x_cl = x.permute(0, 2, 3, 1).contiguous()
    out = {}
    for tile in (1, 2):
        lib.launch_trace()
        with lib.tuning(c2w_tile=tile, c2w_splitk=1):
            out[tile] = ops.conv2d_wide_forward(x_cl, wt, b, relu=True, arith=mode)
        assert lib.launch_trace()[1] == "conv2d_wide %s %s" % (mode, "t64x64" if tile == 1 else "t128x64")
    again = ops.conv2d_wide_forward(x_cl, wt, b, relu=True, arith=mode)
    assert torch.equal(out[1], out[2]) and torch.equal(again, out[1]) and float(again.abs().max()) > 0.1


def test_segdff_routing(dev, vgg):
    from mvs_amd import _lib
    from mvs_amd.jdacs.models.seg_dff import SegDFF
    lib = _lib.get()
    imgs = torch.rand(1, 7, 3, 64, 80, generator=torch.Generator().manual_seed(4)).to(dev)
    lib.launch_trace()
    heat = SegDFF(4, net=vgg, hip_features=True, feature_arith="bf16")(imgs)
    tr = lib.launch_trace()
    assert "resize_cl" in tr and "conv2d_wide cin3" in tr
    assert any(t.startswith("conv2d_wide bf16 t") or t.startswith("conv2d_wide bf16 splitk") for t in tr)
    assert not any(t.startswith("conv2d_wide t") or t.startswith("conv2d_wide splitk") for t in tr)
    assert tuple(heat.shape) == (1, 7, 14, 14, 4) and bool(torch.isfinite(heat).all()) and not heat.requires_grad
    # the default constructor: what it is without this feature
    SegDFF(4, net=vgg)(imgs)
    tr = lib.launch_trace()
    assert not any("bf16" in t for t in tr)
    assert any(t.startswith("conv2d_wide t") or t.startswith("conv2d_wide splitk") for t in tr) == bool(SegDFF.HIP_FEATURES_DEFAULT)


def test_no_host_sync_and_same_bits(dev, vgg):
    """resize + trunk (bf16) + NMF solve under torch.cuda.set_sync_debug_mode("error"); a second run gives the same bits"""
    from mvs_amd import ops
    from mvs_amd.jdacs.models.seg_dff import initial_factors, trunk_layers
    imgs = torch.rand(7, 3, 64, 80, generator=torch.Generator().manual_seed(5)).to(dev)
    layers = [(m.weight, m.bias, relu, pool) for m, relu, pool in trunk_layers(vgg)]
    x = ops.resize_bilinear_cl(imgs, (224, 224))
    flat = ops.conv_trunk_forward(ops.trunk_plan(layers, x.shape, x, arith="bf16"), x).view(1, -1, 512)   # first use: plan, allocator warm-up
    W0, H0 = initial_factors(flat[0], 4, 1)
    W0, H0 = W0.unsqueeze(0), H0.unsqueeze(0)
    ops.nmf_solve(flat, W0, H0)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        torch.cuda.set_sync_debug_mode("error")
        try:
            x = ops.resize_bilinear_cl(imgs, (224, 224))
            flat = ops.conv_trunk_forward(ops.trunk_plan(layers, x.shape, x, arith="bf16"), x).view(1, -1, 512)
            W, H, status = ops.nmf_solve(flat, W0, H0, max_iter=50, tol=1e-4)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        outs.append([t.cpu() for t in (flat, W, H, status)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][1]).all())
