"""GPU (MI355X): the wide forward convolutions and the frozen trunk (csrc/conv2d_wide_kernels.h) on the device.

Every size-selected arm and both sides of both thresholds run at least once with the launch trace asserted; truth = fp64
F.conv2d on the device, yardstick = ATen's fp32 convolution on the device, criterion = conftest's; two calls give the same bits
(no atomics, the split-K sum has a fixed order).  Then the whole VGG19 trunk at full size, SegDFF's routing, and that resize +
trunk + NMF solve are enqueued without a host synchronisation.

Per-case error ratios (ours / ATen fp32, both against fp64; max and mean) are appended to the file MVS_VGG_REPORT names; the copy
kept with the project is profiles/vgg_features_parity_ratios.jsonl."""
import json
import os
import time

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_as_accurate_as_fp32_reference
import seg_oracle as S
from test_vgg_features import LAYER_CASES, expected_conv_labels, layer_inputs, layer_reference

pytestmark = pytest.mark.gpu

KNOBS = ("c2w_tile", "c2w_big_min", "c2w_splitk", "c2w_split_min")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from mvs_amd import _lib
    _lib._INSTANCE = None
    lib = _lib.get()
    assert lib.raw("mvs_is_emulation") == 0  # the product library, not the test emulation
    return torch.device("cuda:0")


def _report(row):
    out = os.environ.get("MVS_VGG_REPORT", "")
    if not out:
        return
    try:
        with open(out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
    except OSError:
        pass


def _ratios(ours, ref32, truth64):
    t = truth64.float()
    eo, er = (ours - t).abs(), (ref32 - t).abs()
    return {"max_ours": float(eo.max()), "max_aten": float(er.max()), "mean_ours": float(eo.mean()), "mean_aten": float(er.mean()),
            "ratio_max": float(eo.max()) / max(float(er.max()), 1e-30), "ratio_mean": float(eo.mean()) / max(float(er.mean()), 1e-30)}


def arm_cases():
    """(case, what it covers); the threshold cases are built from the library's own knob values, one at and one just under each"""
    from mvs_amd import _lib
    lib = _lib.get()
    big, smin = lib.get_tuning("c2w_big_min"), lib.get_tuning("c2w_split_min")
    assert smin % 8 == 0 and 64 <= smin <= 4096 and 64 <= big <= 4096
    cases = [(c, "per-layer case") for c in LAYER_CASES]
    cases += [((1, 14, 14, 512, 512, False), "deepest layer, one image: the most K ranges"),
              ((7, 14, 14, 256, 512, False), "deep layer, seven images"),
              ((1, 56, 56, 128, 256, False), "block 3"),
              ((1, 224, 224, 3, 64, False), "the first layer at full size"),
              ((1, 112, 112, 64, 64, True), "pool at full width"),
              ((1, 128, big, 32, 64, False), "t128x64: exactly c2w_big_min workgroups"),
              ((1, 128, big - 1, 32, 64, False), "one workgroup under c2w_big_min: t64x64"),
              ((1, 8, smin, 64, 512, False), "exactly c2w_split_min t64x64 workgroups: not split"),
              ((1, 8, smin - 8, 64, 512, False), "eight workgroups under c2w_split_min: two K ranges")]
    return cases


def _case_id(c):
    return "%dx%dx%d_%dto%d%s" % (c[:5] + ("_pool" if c[5] else "",))


@pytest.mark.parametrize("idx", range(13))
def test_arm_vs_aten(dev, idx):
    from mvs_amd import _lib, ops
    lib = _lib.get()
    case, what = arm_cases()[idx]
    n, h, w, cin, cout, pool = case
    x, wt, b = [t.to(dev) for t in layer_inputs(case)]
    with torch.no_grad():
        r64 = layer_reference(x, wt, b, True, pool, torch.float64)
        r32 = layer_reference(x, wt, b, True, pool, torch.float32)
    x_cl = x.permute(0, 2, 3, 1).contiguous()
    lib.launch_trace()
    y = ops.conv2d_wide_forward(x_cl, wt, b, relu=True, pool=pool)
    trace = lib.launch_trace()
    y2 = ops.conv2d_wide_forward(x_cl, wt.contiguous(memory_format=torch.channels_last), b, relu=True, pool=pool)
    want = ["conv2d_wide pack"] + expected_conv_labels(n * h * w, cin, cout, big_min=lib.get_tuning("c2w_big_min"),
                                                       split_min=lib.get_tuning("c2w_split_min")) + (["pool2x2"] if pool else [])
    r = _ratios(y, r32, r64)
    print("%s (%s): %s  max %.3e vs ATen %.3e, mean %.3e vs %.3e" % (_case_id(case), what, trace[1], r["max_ours"], r["max_aten"],
                                                                    r["mean_ours"], r["mean_aten"]))
    _report(dict(case=_case_id(case), what=what, arm=trace[1:], **r))
    assert trace == want
    assert torch.equal(y, y2)                  # two calls (the second from a channels-last parameter): the same bits
    assert_as_accurate_as_fp32_reference(y, r32, r64, what=_case_id(case))


def test_arm_cases_cover_every_arm(dev):
    """the list above reaches every label the dispatcher can give under the default knobs"""
    from mvs_amd import _lib
    lib = _lib.get()
    seen = set()
    for (n, h, w, cin, cout, _), _ in arm_cases():
        seen.update(expected_conv_labels(n * h * w, cin, cout, big_min=lib.get_tuning("c2w_big_min"), split_min=lib.get_tuning("c2w_split_min")))
    assert {"conv2d_wide cin3", "conv2d_wide t128x64", "conv2d_wide t64x64", "conv2d_wide splitk=2", "conv2d_wide splitk=4",
            "conv2d_wide splitk=8", "conv2d_wide reduce"} <= seen
    assert len(arm_cases()) == 13


def test_resize_vs_interpolate(dev):
    from mvs_amd import _lib, ops
    x = torch.rand(7, 3, 64, 80, generator=torch.Generator().manual_seed(2)).to(dev)
    _lib.get().launch_trace()
    y = ops.resize_bilinear_cl(x, (224, 224))
    assert _lib.get().launch_trace() == ["resize_cl"]
    r32 = F.interpolate(x, size=(224, 224), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    r64 = F.interpolate(x.double(), size=(224, 224), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert_as_accurate_as_fp32_reference(y, r32, r64, what="resize")


@pytest.fixture(scope="module")
def vgg(dev):
    """vgg19_trunk() of seed 0 with every bias 0.01 randn, on the device"""
    from mvs_amd.jdacs.models.seg_dff import vgg19_trunk
    torch.manual_seed(0)
    net = vgg19_trunk()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.copy_(0.01 * torch.randn(p.shape, generator=g))
    return net.to(dev)


def _trunk(net, x_cl):
    from mvs_amd import ops
    from mvs_amd.jdacs.models.seg_dff import trunk_layers
    plan = ops.trunk_plan([(m.weight, m.bias, relu, pool) for m, relu, pool in trunk_layers(net)], x_cl.shape, x_cl)
    return ops.conv_trunk_forward(plan, x_cl)


def test_whole_trunk_full_size(dev, vgg):
    """VGG19's trunk on 224x224 images.  N = 1: truth = the same network in fp64 on the device, yardstick = the network in fp32
    (ATen / MIOpen), criterion on the [1,14,14,512] output.  N = 7: the batched output against the fp32 yardstick of all seven
    images, with the fp64 truth for image 0 only (the N = 1 input is image 0).

    Is image i of the batched call bitwise the single-image call?  NOT in general: the arm is chosen from N H W (the number of
    workgroups a launch has), and a layer that runs split-K for one image and unsplit for seven adds its K ranges in another
    order.  The tile (t128x64 / t64x64) alone does not change the bits.  Measured on the MI355X: image 0 of the N = 7 call is NOT
    bitwise the N = 1 call (one image runs blocks 2-5 split-K, seven images only block 5).  The test prints what it finds and
    asserts only that the two agree within the criterion.  (The fp64 device forward of one image takes well under a second, so
    the test runs at the full 224x224.)"""
    import copy
    from mvs_amd import _lib
    lib = _lib.get()
    x7 = torch.rand(7, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(dev)
    x1 = x7[:1].contiguous()
    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.time()
        r64 = copy.deepcopy(vgg).double().features(x1.double()).permute(0, 2, 3, 1).contiguous()
        torch.cuda.synchronize()
        print("fp64 device forward of one image: %.2f s" % (time.time() - t0))
        r32_7 = vgg.features(x7).permute(0, 2, 3, 1).contiguous()
        r32_1 = vgg.features(x1).permute(0, 2, 3, 1).contiguous()
    lib.launch_trace()
    y1 = _trunk(vgg, x1.permute(0, 2, 3, 1).contiguous())
    tr1 = lib.launch_trace()
    y7 = _trunk(vgg, x7.permute(0, 2, 3, 1).contiguous())
    tr7 = lib.launch_trace()
    assert tuple(y1.shape) == (1, 14, 14, 512) and tuple(y7.shape) == (7, 14, 14, 512)
    assert float(r64.abs().max()) > 1e-3
    r = _ratios(y1, r32_1, r64)
    print("trunk N=1: max %.3e vs ATen %.3e, mean %.3e vs %.3e; arms %s" % (r["max_ours"], r["max_aten"], r["mean_ours"], r["mean_aten"],
                                                                        [t for t in tr1 if t.startswith("conv2d_wide") and "pack" not in t and "reduce" not in t]))
    _report(dict(case="vgg19 trunk 1x224x224", what="whole trunk", arm=tr1, **r))
    assert_as_accurate_as_fp32_reference(y1, r32_1, r64, what="trunk N=1")
    r = _ratios(y7[:1], r32_7[:1], r64)
    print("trunk N=7, image 0: max %.3e vs ATen %.3e, mean %.3e vs %.3e; arms %s; image 0 bitwise the single-image call: %s"
          % (r["max_ours"], r["max_aten"], r["mean_ours"], r["mean_aten"],
             [t for t in tr7 if t.startswith("conv2d_wide") and "pack" not in t and "reduce" not in t], bool(torch.equal(y7[:1], y1))))
    _report(dict(case="vgg19 trunk 7x224x224 image 0", what="whole trunk", arm=tr7, **r))
    assert_as_accurate_as_fp32_reference(y7[:1], r32_7[:1], r64, what="trunk N=7 image 0")
    # all seven images against the yardstick: the two fp32 evaluations agree within the sum of both errors against the truth
    # (measured on image 0, where the truth exists), with the criterion's slack
    bound = 4.0 * (float((y7[:1] - r64.float()).abs().max()) + float((r32_7[:1] - r64.float()).abs().max())) + 2e-6
    assert float((y7 - r32_7).abs().max()) <= bound


def test_plan_is_per_shape_and_packs_once(dev, vgg):
    from mvs_amd import _lib, ops
    lib = _lib.get()
    x = torch.rand(2, 56, 56, 3, device=dev)
    ops._TRUNK_PLANS.clear()
    lib.launch_trace()
    a = _trunk(vgg, x)
    t0 = lib.launch_trace()
    b = _trunk(vgg, x)
    t1 = lib.launch_trace()
    assert t0.count("conv2d_wide pack") == 16 and t1.count("conv2d_wide pack") == 0 and torch.equal(a, b)


def test_segdff_routing(dev, vgg):
    from mvs_amd import _lib
    from mvs_amd.jdacs.losses.unsup_seg_loss import UnSupSegLoss
    from mvs_amd.jdacs.models.seg_dff import SegDFF
    lib = _lib.get()
    imgs = torch.rand(1, 7, 3, 64, 80, generator=torch.Generator().manual_seed(4)).to(dev)

    def wide(trace):
        return [t for t in trace if t.startswith("conv2d_wide") or t == "resize_cl"]

    lib.launch_trace()
    heat = SegDFF(4, net=vgg, hip_features=True)(imgs)
    tr = lib.launch_trace()
    assert "resize_cl" in tr and any(t.startswith("conv2d_wide t") or t.startswith("conv2d_wide splitk") for t in tr) and "conv2d_wide cin3" in tr
    assert tuple(heat.shape) == (1, 7, 14, 14, 4) and bool(torch.isfinite(heat).all()) and not heat.requires_grad
    stock = SegDFF(4, net=vgg, hip_features=False)(imgs)
    assert wide(lib.launch_trace()) == []
    print("relative L1 of the heat maps of the two routes: %.3e" % float((heat - stock).abs().sum() / stock.abs().sum()))
    # the default follows the measured decision: HIP only where SegDFF.HIP_FEATURES_DEFAULT says so
    SegDFF(4, net=vgg)(imgs)
    assert bool(wide(lib.launch_trace())) == bool(SegDFF.HIP_FEATURES_DEFAULT)
    stand_in = S.StandInNet().to(dev)
    SegDFF(4, net=stand_in)(imgs)
    assert wide(lib.launch_trace()) == []
    with pytest.raises(ValueError, match="hip_features=True"):
        SegDFF(4, net=stand_in, hip_features=True)
    crit = UnSupSegLoss(4, net=vgg, hip_features=True)
    assert crit.seg_model.hip_features is True


def test_no_host_sync_and_same_bits(dev, vgg):
    """resize + trunk + NMF solve run under torch.cuda.set_sync_debug_mode("error") (any host synchronisation raises); a second run
    gives the same bits."""
    from mvs_amd import ops
    from mvs_amd.jdacs.models.seg_dff import initial_factors, trunk_layers
    imgs = torch.rand(7, 3, 64, 80, generator=torch.Generator().manual_seed(5)).to(dev)
    layers = [(m.weight, m.bias, relu, pool) for m, relu, pool in trunk_layers(vgg)]
    x = ops.resize_bilinear_cl(imgs, (224, 224))
    flat = ops.conv_trunk_forward(ops.trunk_plan(layers, x.shape, x), x).view(1, -1, 512)       # first use: plan, allocator warm-up
    W0, H0 = initial_factors(flat[0], 4, 1)
    W0, H0 = W0.unsqueeze(0), H0.unsqueeze(0)
    ops.nmf_solve(flat, W0, H0)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        torch.cuda.set_sync_debug_mode("error")
        try:
            x = ops.resize_bilinear_cl(imgs, (224, 224))
            flat = ops.conv_trunk_forward(ops.trunk_plan(layers, x.shape, x), x).view(1, -1, 512)
            W, H, status = ops.nmf_solve(flat, W0, H0, max_iter=50, tol=1e-4)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        outs.append([t.cpu() for t in (flat, W, H, status)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][1]).all())
